"""dL/d(origins, directions) through PACKED, occupancy-marched samples: the kernel (nrhip_encode_bwd_rays_packed /
ops.encode_bwd_rays_packed), the node that calls it (autograd.NffRenderTrainFn on packed samples with rays that require grad), and the
opt-ins that reach it (NeuRADField.render_train_packed(ray_gradients=True), VolumetricSampler.render_train(
fused_ray_gradients=True)).

The kernel is held per element to the float64 reference and the bound of tests/packed_ray_grad_refs.py on ragged segments,
to the reference's own autograd (tests/golden/ray_grads.npz, ray_grads_edges.npz) exactly as the dense kernel is
(tests/test_gpu_ray_grads.py, tests/test_gpu_position_grad_precision.py), and to what its structure promises: the same bits
run to run and wherever a ray sits in the batch, nothing from exactly-zero rows, a non-finite row confined to its ray."""
import functools

import numpy as np
import pytest
import torch

import neurad_oracle as O
import packed_ray_grad_refs as G
import packed_restatement as PR
import packed_train_refs as T
from conftest import load_golden, rel_l2
from gpu_util import cuda, dev, host, host64_via32, ray_bundle
from gpu_util import ops  # noqa: F401  (fixture)
from grad_edge_refs import edge_g_enc, edge_grid, excess

pytestmark = pytest.mark.gpu

TOL = 1e-4
COUNTS = np.asarray(T.RAGGED, np.int64)
M_RAGGED = int(COUNTS.sum())  # 745
EMPTY = COUNTS == 0
LANES = (16, 32, 64, 0)


def ragged():
    return T.packed_rays(T.RAGGED, 7)


def spec_of(ops, grid):
    return ops.GridSpec(grid.num_levels, grid.n_feat, grid.log2_hashmap_size, grid.min_res, grid.max_res)


def run_packed(ops, grid, scale, rays, ge, tdt=torch.float32, lanes=0, fill=None):
    """the kernel on host arrays -> float64 (grad_origins, grad_directions).  fill: the entry point is called on the
    caller's own buffers, pre-filled with `fill` (the wrapper allocates its outputs itself)"""
    o, d, area, ts, te, seg = rays
    args = (dev(o), dev(d), dev(area), dev(ts), dev(te), cuda(seg))
    table = dev(grid.table).to(tdt)
    if fill is None:
        go, gd = ops.encode_bwd_rays_packed(spec_of(ops, grid), table, scale, *args, dev(ge), lanes_per_ray=lanes)
    else:
        r, keep = ops._c_packed_rays("test", *args)
        go, gd = (torch.full((len(seg) - 1, 3), fill, device="cuda") for _ in range(2))
        ops.launch("nrhip_encode_bwd_rays_packed", spec_of(ops, grid).c_grid(table), table, float(scale), r, dev(ge), lanes,
                   go, gd)
    return host64_via32(go), host64_via32(gd)


@functools.lru_cache(maxsize=None)
def ragged_case(F, half, k):
    """incoming gradients at SCALES[k] and their reference on the ragged batch; shared by the four group sizes"""
    L, _ = G.layout(F)
    ge = G.sharp_gradients(M_RAGGED, L * F, 700 + 10 * F + k, G.SCALES[k])
    return ge, G.reference(G.grid_for(F, half), G.STATIC_SCALE, ragged(), ge)


# ---- 1. per element on ragged segments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("lanes", LANES)
def test_per_element_on_ragged_segments(ops, lanes, F, half):
    """every group size on one batch (counts 0, 1, 15-17, 31-33, 64, 65, 130, 250; first and last ray empty), every F of
    dispatch_f, fp32 and fp16-storage tables (the reference reads the fp16-rounded values), gradients over 16 decades and
    at GradScaler scales; rays without samples: exact zeros WRITTEN over the NaNs the buffers held"""
    L, _ = G.layout(F)
    grid = G.grid_for(F, half)
    gam = G.gamma(COUNTS, lanes, L, F)
    inside = 0
    for k, sc in enumerate(G.SCALES):
        ge, ref = ragged_case(F, half, k)
        go, gd = run_packed(ops, grid, G.STATIC_SCALE, ragged(), ge, torch.float16 if half else torch.float32, lanes,
                            fill=float("nan"))
        assert np.isfinite(go).all() and np.isfinite(gd).all(), (sc, "a row was not written, or is not finite")
        assert (go[EMPTY] == 0).all() and (gd[EMPTY] == 0).all()
        worst = G.worst_excess(go, gd, ref, gam)
        print(f"lanes {lanes} F {F} {'fp16' if half else 'fp32'} scale {sc:g}: worst excess / gamma {worst:.3f}")
        assert worst <= 1.0, (sc, worst)
        inside += int((ref[2][COUNTS >= 15] > 0).all())
    assert inside == len(G.SCALES)  # every ray of 15 samples or more has live terms: the bound is not vacuous
    # the wrapper (its own buffers) returns the same bits
    ge, _ = ragged_case(F, half, 0)
    a = run_packed(ops, grid, G.STATIC_SCALE, ragged(), ge, torch.float16 if half else torch.float32, lanes)
    b = run_packed(ops, grid, G.STATIC_SCALE, ragged(), ge, torch.float16 if half else torch.float32, lanes, fill=7.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_batch_without_samples_and_without_rays(ops):
    grid = G.grid_for(4, False)
    o, d, area, _, _, _ = T.packed_rays((0,) * 7, 3)
    none = np.zeros((0,), np.float32)
    rays = (o, d, area, none, none, np.zeros(8, np.int64))
    go, gd = run_packed(ops, grid, 100.0, rays, np.zeros((0, 32), np.float32), fill=float("nan"))
    assert go.shape == (7, 3) and (go == 0).all() and (gd == 0).all()
    go, gd = run_packed(ops, grid, 100.0, (o[:0], d[:0], area[:0], none, none, np.zeros(1, np.int64)),
                        np.zeros((0, 32), np.float32))
    assert go.shape == (0, 3) and gd.shape == (0, 3)


# ---- 2. the reference's own autograd -----------------------------------------------------------------------------------
def as_segments(g):
    """a fixture's [R,S] batch as uniform segments"""
    R, S = g["starts"].shape
    return (g["o"], g["d"], g["area"], np.ascontiguousarray(g["starts"]).reshape(-1), np.ascontiguousarray(g["ends"]).reshape(-1),
            PR.segments_from_counts([S] * R))


def test_vs_reference_autograd(ops):
    """tests/golden/ray_grads.npz (40 x 24) fed as uniform segments: the dense test's bound"""
    g = load_golden("ray_grads")
    grid = G.grid_for(4, False)  # the fixture's table: seed 51, 8 x 4 on 2^11
    for lanes in LANES:
        go, gd = run_packed(ops, grid, 100.0, as_segments(g), g["g_enc"], lanes=lanes)
        assert rel_l2(go, g["enc_go"]) < TOL and rel_l2(gd, g["enc_gd"]) < TOL, lanes


def test_edges(ops):
    """E1-E3 rows of tests/golden/ray_grads_edges.npz (156 x 8) through the packed kernel, held as
    test_gpu_position_grad_precision.test_encode_bwd_rays_edges holds the dense one: the float64 oracle within gamma, the
    reference's autograd within gamma + 2, and the wrong subgradients outside the bound on those rows"""
    g = load_golden("ray_grads_edges")
    grid, sc = edge_grid(), float(g["static_scale"])
    args = (g["o"], g["d"], g["area"], g["starts"], g["ends"])
    ge = edge_g_enc(g)
    ref_o, ref_d, ao, ad = O.encode_static_ray_grads(grid, sc, *args, ge, with_abs=True)
    R, S = g["starts"].shape
    gam = float(G.gamma([S] * R, 0, 8, 4).max())
    assert gam == 48 + 4 + 8 + 1 + 4  # the dense test's gamma_rays(S, 8, 4): 16 lanes, one sample per lane
    k = g["kind"]
    for tdt in (torch.float32, torch.float16):
        if tdt == torch.float16:
            grid = O.GridParams(grid.table.astype(np.float16).astype(np.float32), 8, 32, 8192, 11)
            ref_o, ref_d, ao, ad = O.encode_static_ray_grads(grid, sc, *args, ge, with_abs=True)
        go, gd = run_packed(ops, grid, sc, as_segments(g), ge, tdt)
        for got, ref, A in ((go, ref_o, ao), (gd, ref_d, ad)):
            assert excess(got, ref, A).max() <= gam, excess(got, ref, A).max()
        if tdt == torch.float32:  # the fixture was made with the fp32 table
            for got, ref, A in ((go, g["enc_go"], ao), (gd, g["enc_gd"], ad)):
                assert excess(got, ref, A).max() <= gam + 2, excess(got, ref, A).max()
    for ties, clamp, kinds in (("first", True, (1, 2, 3)), ("split", False, (3,))):
        bo, bd = O.encode_static_ray_grads(grid, sc, *args, ge, ties=ties, clamp_at_one=clamp)
        for kk in kinds:
            worst = max(excess(bo, ref_o, ao)[k == kk].max(), excess(bd, ref_d, ad)[k == kk].max())
            assert worst > 10 * gam, (ties, clamp, kk, worst)


# ---- 3. reproducible and order-free ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_reproducible_and_independent_of_the_rays_place(ops, lanes):
    grid = G.grid_for(4, False)
    ge, _ = ragged_case(4, False, 0)
    a = run_packed(ops, grid, G.STATIC_SCALE, ragged(), ge, lanes=lanes)
    b = run_packed(ops, grid, G.STATIC_SCALE, ragged(), ge, lanes=lanes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # no atomics: the same bits
    perm = np.random.default_rng(5).permutation(len(COUNTS))
    assert (perm != np.arange(len(COUNTS))).sum() > 15
    rays_p, take = G.permuted(ragged(), perm)
    c = run_packed(ops, grid, G.STATIC_SCALE, rays_p, ge[take], lanes=lanes)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm])


def test_exactly_zero_rows_contribute_nothing(ops):
    grid = G.grid_for(4, False)
    ge = ragged_case(4, False, 0)[0].copy()
    ge[::3] = 0
    ref = G.reference(grid, G.STATIC_SCALE, ragged(), ge)
    for lanes in LANES:
        go, gd = run_packed(ops, grid, G.STATIC_SCALE, ragged(), ge, lanes=lanes)
        assert G.worst_excess(go, gd, ref, G.gamma(COUNTS, lanes, 8, 4)) <= 1.0, lanes
    one = COUNTS == 1  # a ray whose only sample is silent: zeros
    first = PR.segments_from_counts(COUNTS)[:-1]
    silent = one & (first % 3 == 0)
    assert silent.any() and (go[silent] == 0).all() and (gd[silent] == 0).all()


# ---- 4. containment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [16, 64, 0])
def test_non_finite_row_stays_in_its_ray(ops, lanes):
    """a NaN or inf in one sample's row makes that ray's gradient non-finite and leaves every other ray in its bound"""
    grid = G.grid_for(4, False)
    ge, ref = ragged_case(4, False, 0)
    seg = PR.segments_from_counts(COUNTS)
    gam = G.gamma(COUNTS, lanes, 8, 4)
    for bad, ray in ((np.nan, 14), (np.inf, 20), (np.nan, 1)):  # 130 samples, 250 samples, a single sample
        gb = ge.copy()
        gb[seg[ray] + COUNTS[ray] // 2, 3] = bad
        go, gd = run_packed(ops, grid, G.STATIC_SCALE, ragged(), gb, lanes=lanes)
        others = np.arange(len(COUNTS)) != ray
        assert not np.isfinite(go[ray]).all() and not np.isfinite(gd[ray]).all()
        assert np.isfinite(go[others]).all() and np.isfinite(gd[others]).all()
        assert G.worst_excess(go, gd, ref, gam, rows=others) <= 1.0


# ---- 5. the node -------------------------------------------------------------------------------------------------------
def node_step(fld, dr, cot, ray_grads):
    o, d = dr[0].clone().requires_grad_(ray_grads), dr[1].clone().requires_grad_(ray_grads)
    outs = fld.render_train_packed(o, d, *dr[2:5], segments=dr[5], ray_gradients=ray_grads)
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    return [t.detach() for t in outs], T.field_grads(fld), o.grad, d.grad


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("batch", ["ragged", "large"])
def test_node_returns_the_kernels_gradients(ops, batch, use_sdf, monkeypatch):
    rays = ragged() if batch == "ragged" else G.large_rays()
    dr = T.on_device(rays)
    R, M = len(rays[5]) - 1, rays[3].shape[0]
    assert (M >= ops._BINNED_MIN_SAMPLES) == (batch == "large")  # the table gradient: partition path / atomic scatter
    cot = G.cotangents(R, M)
    calls = []
    real = ops.encode_bwd_rays_packed

    def spy(spec, table, scale, o, d, a, ts, te, seg, grad_out, lanes_per_ray=0):
        out = real(spec, table, scale, o, d, a, ts, te, seg, grad_out, lanes_per_ray)
        calls.append((grad_out.detach().clone(), out[0].clone(), out[1].clone()))
        return out

    monkeypatch.setattr(ops, "encode_bwd_rays_packed", spy)
    fld, p = T.make_field(8, 4, 32, use_sdf)
    outs, grads, go, gd = node_step(fld, dr, cot, True)
    assert len(calls) == 1
    genc, ko, kd = calls[0]
    assert go.shape == (R, 3) and torch.equal(go, ko) and torch.equal(gd, kd)
    # the dL/d enc the backward formed, through the float64 reference
    ref = G.reference(p.grid, 100.0, rays, host(genc))
    counts = np.diff(rays[5])
    worst = G.worst_excess(host64_via32(go), host64_via32(gd), ref, G.gamma(counts, 0, 8, 4))
    print(f"{batch} {'sdf' if use_sdf else 'density'}: worst excess / gamma {worst:.3f}")
    assert worst <= 1.0 and float(go.abs().sum()) > 0 and float(gd.abs().sum()) > 0
    assert bool((go[torch.from_numpy(counts == 0).cuda()] == 0).all())
    # the same step with fixed rays: the same outputs and parameter gradients, no ray-gradient launch
    fld2, _ = T.make_field(8, 4, 32, use_sdf)
    outs2, grads2, go2, gd2 = node_step(fld2, dr, cot, False)
    assert len(calls) == 1 and go2 is None and gd2 is None
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    assert set(grads) == set(grads2) and ("sdf_to_density.beta" in grads) == use_sdf
    for n in grads:
        if batch == "large":
            assert torch.equal(grads[n], grads2[n]), n
        else:  # (a batch this small takes the atomic scatter)
            assert rel_l2(host(grads[n]).reshape(-1), host(grads2[n]).reshape(-1)) < 1e-6, n


def test_node_with_one_of_the_two_requiring_grad(ops):
    dr = T.on_device(ragged())
    cot = G.cotangents(len(COUNTS), M_RAGGED)
    fld, _ = T.make_field(8, 4, 32, True)
    _, _, go, gd = node_step(fld, dr, cot, True)
    for which in (0, 1):
        f2, _ = T.make_field(8, 4, 32, True)
        o, d = dr[0].clone().requires_grad_(which == 0), dr[1].clone().requires_grad_(which == 1)
        outs = f2.render_train_packed(o, d, *dr[2:5], segments=dr[5], ray_gradients=True)
        sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
        assert (o.grad is None) == (which == 1) and (d.grad is None) == (which == 0)
        assert torch.equal(o.grad, go) if which == 0 else torch.equal(d.grad, gd)


# ---- 6. against the route it replaces ------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_sampler_opt_in_vs_the_fallback(ops, use_sdf, monkeypatch):
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    R = 96
    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    est.binaries[0] = dev(np.random.default_rng(3).random((16, 16, 16)) < 0.3)
    sampler = VolumetricSampler(est).train()
    kw = dict(render_step_size=0.1, cone_angle=0.0)
    keys = {"features", "depth", "accumulation", "weights", "ray_indices", "t_starts", "t_ends"}

    def refuse(*a, **k):
        raise AssertionError("the wrong route ran")

    def moving_bundle():
        rb = ray_bundle(R, 90, far=9.0)
        rb.origins.requires_grad_(True), rb.directions.requires_grad_(True)
        return rb

    fld, _ = T.make_field(8, 4, 32, use_sdf)
    rb = moving_bundle()
    with monkeypatch.context() as m:  # the node reads the bundle's own tensors: no gather of the ray constants
        m.setattr(VolumetricSampler, "_gather", staticmethod(refuse))
        got = sampler.render_train(fld, rb, fused_ray_gradients=True, **kw)
    assert set(got) == keys
    ri, ts, te = got["ray_indices"], got["t_starts"], got["t_ends"]
    M = ri.shape[0]
    counts = torch.bincount(ri, minlength=R)
    assert M > 1000 and int((counts == 0).sum()) >= 4 and got["weights"].shape == (M, 1)
    cot = G.cotangents(R, M, 91)
    outs = [got[k] for k in ("features", "depth", "accumulation", "weights")]
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    fused = ([t.detach().reshape(c.shape) for t, c in zip(outs, cot)], T.field_grads(fld))
    # the fallback fed the RETURNED samples (the stratified draw is shared), rays requiring grad
    fld2, _ = T.make_field(8, 4, 32, use_sdf)
    rb2 = moving_bundle()
    op_outs = T.operator_route(fld2, (rb2.origins, rb2.directions, rb2.pixel_area.reshape(-1), ts, te, None, ri))
    assert [tuple(t.shape) for t in op_outs] == [tuple(c.shape) for c in cot]
    sum((t * c).sum() for t, c in zip(op_outs, cot)).backward()
    G.compare_routes(fused, ([t.detach() for t in op_outs], T.field_grads(fld2)))
    live = (counts > 0).cpu().numpy()
    for name, a, c in (("origins", rb.origins.grad, rb2.origins.grad), ("directions", rb.directions.grad, rb2.directions.grad)):
        a, c = host(a).astype(np.float64), host(c).astype(np.float64)
        assert (a[~live] == 0).all() and (c[~live] == 0).all()
        per_ray = np.linalg.norm(a[live] - c[live], axis=-1) / np.linalg.norm(c[live], axis=-1)
        print(f"d {name}: node vs fallback per ray: median {np.median(per_ray):.3e}, worst {per_ray.max():.3e}")
        # (measured on an MI355X: median 1.4e-7 / 1.4e-7 (SDF head), 1.6e-7 / 1.7e-7 (density head); worst ray 1.2e-6)
        assert np.median(per_ray) < 1e-3, (name, np.sort(per_ray)[-5:])
    # the default: rays that require grad still take the fallback
    f3, _ = T.make_field(8, 4, 32, use_sdf)
    rb3 = moving_bundle()
    with monkeypatch.context() as m:
        m.setattr(f3, "render_train_packed", refuse)
        out3 = sampler.render_train(f3, rb3, **kw)
    assert set(out3) == keys
    (out3["features"].sum() + out3["depth"].sum()).backward()
    assert rb3.origins.grad is not None and bool(torch.isfinite(rb3.origins.grad).all())
    # fixed rays: the flag changes nothing (no ray gradient is asked for)
    f4, _ = T.make_field(8, 4, 32, use_sdf)
    rb4 = ray_bundle(R, 90, far=9.0)
    with monkeypatch.context() as m:
        m.setattr(ops, "encode_bwd_rays_packed", refuse)
        out4 = sampler.render_train(f4, rb4, fused_ray_gradients=True, **kw)
        (out4["features"].sum() + out4["depth"].sum()).backward()
    assert rb4.origins.grad is None


# ---- 7. graph replay -----------------------------------------------------------------------------------------------------
def test_node_with_ray_gradients_replays_in_a_graph(ops):
    rays = G.large_rays()  # (the partition source: the small batch's table gradient is formed by memory-side atomics)
    dr = T.on_device(rays)
    M = rays[3].shape[0]
    cot = G.cotangents(1500, M)
    fld, _ = T.make_field(8, 4, 32, True)
    ps = [p for p in fld.parameters() if p.requires_grad]
    o, d = dr[0].clone().requires_grad_(True), dr[1].clone().requires_grad_(True)

    def step():
        outs = fld.render_train_packed(o, d, *dr[2:5], segments=dr[5], ray_gradients=True)
        loss = sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot))
        grads = torch.autograd.grad(loss, [*ps, o, d], allow_unused=True)
        assert grads[-1] is not None and grads[-2] is not None
        return [*outs, *[g for g in grads if g is not None]]

    eager = [t.detach().clone() for t in step()]
    assert float(eager[-1].abs().sum()) > 0 and float(eager[-2].abs().sum()) > 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert len(captured) == len(eager)
        for a, b in zip(eager, captured):
            assert torch.equal(a, b.detach())
