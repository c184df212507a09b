"""The occupancy route with dynamic actors: the box-aware march (nrhip_occgrid_march_levels_actors / ops.occgrid_march(...,
actor_boxes=...)), the fused packed render with actors (nrhip_render_fwd_packed_actors / NeuRADField.render_packed(...,
times=...)) and VolumetricSampler(..., actor_boxes=True).

Scenes, fields and references: tests/packed_actor_refs.py.  Bounds: TOL = 1e-4 rel-L2 against the numpy oracle (the bound of
tests/test_gpu_actors.py), 1e-5 between the fused and the operator route (the bound of tests/test_gpu_render_packed.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import packed_actor_refs as PA
import packed_restatement as PR
from conftest import rel_l2
from gpu_util import TOL, cuda, host
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def cand_lists(fld, s):
    """(spec, per-ray candidate lists) of scene dict / ray tuple `s` at the rays' times"""
    o, d, times = (s["o"], s["d"], s["times"]) if isinstance(s, dict) else (s[0], s[1], s[3])
    return fld.hashgrid.prepare_actors_line(cuda(o), cuda(d), 0.0, 1.0, cuda(times))


# ---- 1. the march ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_field():
    return PA.make_actor_field("golden")[0]


@functools.lru_cache(maxsize=None)
def street_field():
    return PA.make_actor_field("street")[0]


@pytest.mark.parametrize("cone", [0.0, 0.004], ids=["uniform", "cone"])
@pytest.mark.parametrize("stratified", [False, True], ids=["fixed", "stratified"])
@pytest.mark.parametrize("levels", [1, 3], ids=["1-level", "3-levels"])
@pytest.mark.parametrize("name", ["golden", "street"])
def test_march_keeps_the_cells_and_the_boxes(ops, name, levels, stratified, cone):
    """C = the plain march on all-one binaries; the box-aware march returns exactly the c in C that the plain march on the
    same binaries keeps or that the field's own in-box test (ops.actor_encode's hit) puts inside a box: same rays, same
    order, t_starts / t_ends bitwise -- march and field call the same device functions, so no near-face exclusions."""
    s = PA.scene(name)
    fld = golden_field() if name == "golden" else street_field()
    o, d, area = cuda(s["o"]), cuda(s["d"]), cuda(s["area"])
    R = o.shape[0]
    spec, cand = cand_lists(fld, s)
    boxes = torch.from_numpy(PA.level_boxes(s["box0"], levels))
    binaries = cuda(PA.random_binaries(levels, 16, 11 + levels))
    t_rand = cuda(np.random.default_rng(5).random(R).astype(np.float32)) if stratified else None
    kw = dict(render_step_size=s["step"], near_plane=0.1, far_plane=120.0, cone_angle=cone, t_rand=t_rand)
    grid = ops.OccGridSpec(boxes, binaries)
    every = ops.occgrid_march(ops.OccGridSpec(boxes, torch.ones_like(binaries)), o, d, **kw)
    plain = ops.occgrid_march(grid, o, d, **kw)
    got = ops.occgrid_march(grid, o, d, **kw, actor_boxes=(spec, cand))
    hit = host(PA.sample_hits(ops, spec, cand, o, d, area, *every[:3])) >= 0
    cell = np.isin(PA.sample_keys(host(every[0]), host(every[1])), PA.sample_keys(host(plain[0]), host(plain[1])))
    assert cell.sum() == plain[0].shape[0]  # the plain march is a subset of the candidates, bit for bit
    classes = PA.march_classes(cell, hit)
    print("cell only / box only / both / neither:", classes)
    assert all(c > 0 for c in classes), classes
    keep = torch.from_numpy(cell | hit).cuda()
    for g, e in zip(got[:3], every[:3]):
        assert torch.equal(g, e[keep])
    # the count and the write pass agree
    assert int(got[3][-1]) == got[0].shape[0] and torch.equal(got[3], ops.packed_segments(got[0], R))
    # no candidates: the plain march, bit for bit
    none = (torch.zeros_like(cand[0]), cand[1], cand[2], None)
    for g, p in zip(ops.occgrid_march(grid, o, d, **kw, actor_boxes=(spec, none)), plain):
        assert torch.equal(g, p)


# ---- 2. the fused kernel on ragged segments ----------------------------------------------------------------------------------
N_RAGGED = 64


@functools.lru_cache(maxsize=None)
def ragged_case(L, F, H, half):
    """field, rays, oracle outputs, operator-route outputs of one shape: computed once, shared, left unchanged"""
    fld, p, ap = PA.make_actor_field("street", L, F, H, half)
    rays = PA.ragged_rays("street", N_RAGGED, 7)
    return fld, rays, PA.oracle_route(p, ap, rays), PA.operator_route(fld, rays)


RAGGED_CASES = [(L, F, H, half) for L, F, H in PA.SHAPES for half in (False, True)]


@pytest.mark.parametrize("with_order", [False, True], ids=["batch-order", "ray-order"])
@pytest.mark.parametrize("L,F,H,half", RAGGED_CASES, ids=[f"{L}x{F}-H{H}{'-fp16' if h else ''}" for L, F, H, h in RAGGED_CASES])
def test_ragged_segments_every_actor_shape(ops, L, F, H, half, with_order):
    fld, rays, oracle, operator = ragged_case(L, F, H, half)
    assert fld.fused_packed_actors_supported() and not fld.fused_packed_supported()
    o, d, area, times, ts, te, seg = (cuda(a) for a in rays)
    R, M = o.shape[0], ts.shape[0]
    counts = np.diff(rays[6])
    spec, cand = cand_lists(fld, rays)
    cnt = host(cand[0])
    # the batch is what the issue asks for: the segment lengths, rays with and without candidates interleaved, a ray with
    # candidates and no samples, a 16-sample tile with samples in different boxes
    assert {0, 1, 15, 16, 17, 33} <= set(counts.tolist()) and counts.max() > 64
    with_c = cnt > 0
    assert (with_c[1:] != with_c[:-1]).sum() >= 10 and ((counts == 0) & with_c).any() and ((counts > 0) & ~with_c).any()
    hit = host(PA.sample_hits(ops, spec, cand, o, d, area, cuda(PR.ray_indices_from_segments(rays[6])), ts, te))
    tiles = [hit[b + 16 * k:min(b + 16 * k + 16, e)] for b, e in zip(rays[6][:-1], rays[6][1:]) for k in range((e - b + 15) // 16)]
    assert any(len(set(t[t >= 0].tolist())) >= 2 for t in tiles), "one tile must hold samples of different boxes"
    order = ops.ray_order(o, d, 100.0) if with_order else None
    out = (torch.full((R, 32), float("nan"), device="cuda"), torch.full((R, 1), float("nan"), device="cuda"),
           torch.full((R, 1), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda"))
    got = ops.render_fwd_packed_actors(fld.field_spec(), spec, cand, o, d, area, ts, te, seg, return_weights=True, order=order,
                                       out=out)
    assert all(g.data_ptr() == b.data_ptr() for g, b in zip(got, out)) and all(bool(torch.isfinite(g).all()) for g in got)
    PA.close(got, oracle, TOL, "vs oracle")
    PA.close(got, operator, 1e-5, "vs operator route")
    empty = torch.from_numpy(counts == 0).cuda()
    for t in got[:3]:
        assert bool((t[empty] == 0).all())
    # the module's entry: the same bits, with and without the weights
    via_field = PA.fused_route(fld, rays, order=order)
    for a, b in zip(via_field, got):
        assert torch.equal(a.reshape(-1), b.reshape(-1))


# ---- 3. uniform segments against the dense actor kernel -------------------------------------------------------------------------
def test_uniform_segments_against_the_dense_actor_kernel(ops):
    """Every segment S samples long: the dense actor kernel's arithmetic with another addressing.  Its features carry the sky
    residual (1 - acc) x the last sample's feature and its depth leaves the last sample out; both are removed with the
    operator route's per-sample feature."""
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames
    from conftest import load_golden

    g = load_golden("field_actors")
    fld = golden_field()
    R, S = g["starts"].shape
    o, d, area, times, st, en = (cuda(g[k]) for k in ("o", "d", "area", "times", "starts", "ends"))
    seg = torch.arange(R + 1, device="cuda") * S
    with torch.no_grad():
        got = fld.render_packed(o, d, area, st.reshape(-1), en.reshape(-1), segments=seg, times=times, return_weights=True)
        df, dd, da, dw = fld.render(o, d, area, st, en, return_weights=True, times=times)
        rb = RayBundle(origins=o, directions=d, pixel_area=area[:, None], times=times[:, None])
        feat = fld(rb.get_ray_samples(st[..., None], en[..., None]))[FieldHeadNames.FEATURE]  # [R,S,32]
    assert int((cand_lists(fld, PA.scene("golden"))[1][0] > 0).sum()) > 0
    assert rel_l2(host(got[3]), host(dw).reshape(-1)) < 1e-6 and rel_l2(host(got[2]), host(da)) < 1e-6
    want_f = df - (1.0 - da) * feat[:, -1]
    want_d = dd + dw[:, -1:] * (st[:, -1:] + en[:, -1:]) / 2
    assert rel_l2(host(got[0]), host(want_f)) < 1e-5 and rel_l2(host(got[1]), host(want_d)) < 1e-5


# ---- 4. determinism and early stop -------------------------------------------------------------------------------------------
def test_determinism_and_early_termination(ops):
    fld = street_field()
    counts = tuple([96, 40, 130, 7, 0, 64, 33, 16] * 12)
    rays = PA.ragged_rays("street", len(counts), 31, counts=counts)
    first = PA.fused_route(fld, rays)
    for a, b in zip(PA.fused_route(fld, rays), first):
        assert torch.equal(a, b)
    perm = cuda(np.random.default_rng(23).permutation(len(counts)).astype(np.int32))
    for a, b in zip(PA.fused_route(fld, rays, order=perm), first):
        assert torch.equal(a, b)
    # the rays themselves permuted: every ray's outputs keep their bits
    p = np.random.default_rng(29).permutation(len(counts))
    seg = rays[6]
    moved = (rays[0][p], rays[1][p], rays[2][p], rays[3][p],
             np.concatenate([rays[4][seg[r]:seg[r + 1]] for r in p]), np.concatenate([rays[5][seg[r]:seg[r + 1]] for r in p]),
             PR.segments_from_counts(np.diff(seg)[p]))
    again = PA.fused_route(fld, moved)
    pt = torch.from_numpy(p).cuda()
    for a, b in zip(again[:3], first[:3]):
        assert torch.equal(a, b[pt])
    # early termination: bounded as on the static packed kernel
    eps = 1e-3
    with torch.no_grad():
        fld.sdf_to_density.beta.fill_(6.0)
    try:
        f0, d0, a0, w0 = PA.fused_route(fld, rays)
        f1, d1, a1, w1 = PA.fused_route(fld, rays, early_stop_eps=eps)
        exact = PA.fused_route(fld, rays, early_stop_eps=0.0)
    finally:
        with torch.no_grad():
            fld.sdf_to_density.beta.fill_(3.0)
        fld.invalidate_caches()
    cut = (w1 == 0) & (w0 != 0)
    assert float(cut.float().mean()) > 0.25, "the scene must terminate rays early"
    assert torch.equal(w1[~cut], w0[~cut])  # in front of the cut: the same bits
    assert float((a1 - a0).abs().max()) < eps
    assert float((f1 - f0).abs().max()) <= 3 * eps * float(f0.abs().max())
    for a, b in zip(exact, (f0, d0, a0, w0)):
        assert torch.equal(a, b)


# ---- 5. degenerate batches -----------------------------------------------------------------------------------------------------
def test_degenerate_batches(ops):
    fld = street_field()
    fs = fld.field_spec()
    rays = PA.ragged_rays("street", 40, 7)
    o, d, area, times, ts, te, seg = (cuda(a) for a in rays)
    spec, cand = cand_lists(fld, rays)
    # M = 0: zeros, no sample pointer is read
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    f, dp, a, w = ops.render_fwd_packed_actors(fs, spec, cand, o, d, area, z(0), z(0), torch.zeros_like(seg), return_weights=True)
    assert f.shape == (40, 32) and w.shape == (0,) and bool((f == 0).all()) and bool((dp == 0).all()) and bool((a == 0).all())
    # R = 0: a no-op
    A = cand[1].shape[1]
    none = (torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros((0, A), dtype=torch.int32, device="cuda"), z(0, A, 12), None)
    f, dp, a, w = ops.render_fwd_packed_actors(fs, spec, none, z(0, 3), z(0, 3), z(0), z(0), z(0),
                                               torch.zeros(1, dtype=torch.int64, device="cuda"), return_weights=True)
    assert f.shape == (0, 32) and dp.shape == (0, 1) and a.shape == (0, 1) and w.shape == (0,)
    # no candidates anywhere: the static packed kernel, bit for bit
    zero = (torch.zeros_like(cand[0]), cand[1], cand[2], None)
    for x, y in zip(ops.render_fwd_packed_actors(fs, spec, zero, o, d, area, ts, te, seg, return_weights=True),
                    ops.render_fwd_packed(fs, o, d, area, ts, te, seg, return_weights=True)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):  # one list per ray, not per sample
        ops.render_fwd_packed_actors(fs, spec, (cand[0][:-1], cand[1][:-1], cand[2][:-1], None), o, d, area, ts, te, seg)
    # K smaller than the actors on a ray: nrhip_actor_prepare sets its overflow flag and keeps the K lowest actor indices;
    # the kernel walks rows of length K and renders what a full-length list cut to its first K entries renders
    K = 4
    assert int(cand[0].max()) > K
    a_full, keep = spec.c_actors()
    a_k = type(a_full)()
    ctypes.pointer(a_k)[0] = a_full
    a_k.max_candidates = K
    R = o.shape[0]
    edges = torch.stack([z(R), torch.ones(R, device="cuda")], 1)
    r2, keep_r = ops._c_rays(o, d, z(R), edges, edges)
    cnt = torch.empty((R,), dtype=torch.int32, device="cuda")
    act = torch.zeros((R, K), dtype=torch.int32, device="cuda")
    w2b = z(R, K, 12)
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ops.launch("nrhip_actor_prepare", a_k, r2, times, cnt, act, w2b, flag)
    assert int(flag) == 1 and torch.equal(cnt, cand[0].clamp_max(K))
    assert torch.equal(act, cand[1][:, :K].contiguous() * (torch.arange(K, device="cuda")[None] < cnt[:, None]))
    f_, keep_f = fs.c_field()
    pr, keep_p = ops._c_packed_rays("test", o, d, area, ts, te, seg)
    outs = [torch.empty((R, 32), device="cuda"), torch.empty((R, 1), device="cuda"), torch.empty((R, 1), device="cuda"),
            torch.empty_like(ts)]
    work = torch.empty((R + 4,), dtype=torch.int32, device="cuda")
    ops.launch("nrhip_render_fwd_packed_actors", f_, a_k, pr, cnt, act, w2b, *outs, 0.0, work)
    cut = (cand[0].clamp_max(K), cand[1], cand[2], None)
    for x, y in zip(outs, ops.render_fwd_packed_actors(fs, spec, cut, o, d, area, ts, te, seg, return_weights=True)):
        assert torch.equal(x, y)
    # ... and the march with the short rows keeps what the cut lists keep
    s = PA.scene("street")
    grid = ops.OccGridSpec(torch.from_numpy(PA.level_boxes(s["box0"], 1)), cuda(np.zeros((1, 16, 16, 16), bool)))
    want = ops.occgrid_march(grid, o, d, 0.5, 0.1, 120.0, actor_boxes=(spec, cut))
    g_, keep_g = grid.c_levels()
    counts = torch.zeros((R,), dtype=torch.int32, device="cuda")
    ops.launch("nrhip_occgrid_march_levels_actors", g_, a_k, cnt, act, w2b, o, d, None, None, None, R, 0.5, 0.1, 120.0, 0.0,
               1 << 16, counts, None, None, None, None)
    assert want[0].shape[0] > 0 and torch.equal(counts.long(), want[3][1:] - want[3][:-1])


# ---- 6. + 7. the sampler ---------------------------------------------------------------------------------------------------------
def static_grid(name, levels=1, res=32):
    """an estimator as a grid trained on the static density has it: random cells, none inside the actors' boxes"""
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    s = PA.scene(name)
    boxes = PA.level_boxes(s["box0"], 3)
    est = OccGridEstimator(boxes[2].tolist(), resolution=res)
    binaries = PA.random_binaries(1, res, 3)[0]
    lo, hi = boxes[2][:3], boxes[2][3:]
    centres = np.stack(np.meshgrid(*[lo[a] + (np.arange(res) + 0.5) * (hi[a] - lo[a]) / res for a in range(3)], indexing="ij"), -1)
    ap = PA.oracle_actor_params(name)
    pos = ap.positions.reshape(-1, 3)  # every actor at every stored time
    near = (np.linalg.norm(centres[..., None, :] - pos, axis=-1) < 5.0).any(-1)
    binaries &= ~near
    est.binaries[0] = cuda(binaries)
    return est


def operator_render(sampler, fld, rb, monkeypatch, **kw):
    with monkeypatch.context() as m:
        m.setattr(type(fld), "fused_packed_actors_supported", lambda self: False)
        return sampler.render(fld, rb, **kw)


def test_sampler_renders_the_actors_the_static_grid_misses(ops, monkeypatch):
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.model_components.renderers import render_packed

    s = PA.scene("golden")
    fld = golden_field()
    rb = PA.bundle_of((s["o"], s["d"], s["area"], s["times"]))
    R = s["o"].shape[0]
    sampler = VolumetricSampler(static_grid("golden")).eval()
    kw = dict(render_step_size=0.25, near_plane=0.1, far_plane=120.0)
    # the default call: what it was -- the plain march + the operator route, computed here
    o, d, area = rb.origins, rb.directions, rb.pixel_area
    ri, ts, te, seg = ops.occgrid_march(sampler.occupancy_grid._spec(), o, d, 0.25, 0.1, 120.0)
    with torch.no_grad():
        rs = VolumetricSampler._gather(rb, o, d, ri, ts, te)
        out = fld(rs)
        want = render_packed(out[FieldHeadNames.FEATURE], rs, ri, R, alpha=out[FieldHeadNames.ALPHA])
    default = sampler.render(fld, rb, **kw)
    assert torch.equal(default["ray_indices"], ri) and torch.equal(default["t_starts"], ts) and torch.equal(default["t_ends"], te)
    for k in ("features", "depth", "accumulation", "weights"):
        assert torch.equal(default[k], want[k]), k
    # with the boxes: the march keeps the samples inside them, the fused kernel renders them
    spec, cand = cand_lists(fld, s)
    got = sampler.render(fld, rb, **kw, actor_boxes=True)
    hit = PA.sample_hits(ops, spec, cand, o, d, area, got["ray_indices"], got["t_starts"], got["t_ends"]) >= 0
    plain_hit = PA.sample_hits(ops, spec, cand, o, d, area, ri, ts, te) >= 0
    assert int(hit.sum()) > 50 and int(plain_hit.sum()) == 0  # the static grid alone loses every in-box sample
    through = torch.zeros(R, dtype=torch.bool, device="cuda")
    through[got["ray_indices"][hit]] = True
    assert int(through.sum()) >= 10 and bool((got["accumulation"][through, 0] > 0).all())
    only_box = through & (default["accumulation"][:, 0] == 0)
    print("rays through a box:", int(through.sum()), " of them without any other sample:", int(only_box.sum()))
    op = operator_render(sampler, fld, rb, monkeypatch, **kw, actor_boxes=True)
    for k in ("ray_indices", "t_starts", "t_ends"):
        assert torch.equal(op[k], got[k])
    PA.close([got[k] for k in ("features", "depth", "accumulation", "weights")],
             [op[k] for k in ("features", "depth", "accumulation", "weights")], 1e-5, "fused vs operator route")


def test_actor_edit_moves_march_and_render_together(ops, monkeypatch):
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler

    s = PA.scene("golden")
    fld = PA.make_actor_field("golden")[0]  # (its own: the edit is state)
    rb = PA.bundle_of((s["o"], s["d"], s["area"], s["times"]))
    sampler = VolumetricSampler(static_grid("golden")).eval()
    kw = dict(render_step_size=0.25, near_plane=0.1, far_plane=120.0, actor_boxes=True)
    before = sampler.render(fld, rb, **kw)
    fld.hashgrid.actors.actor_editing.update(lateral=1.5, longitudinal=-2.0, height=0.3, rotation=0.4, index=-1.0)
    got = sampler.render(fld, rb, **kw)
    assert got["t_starts"].shape != before["t_starts"].shape or not torch.equal(got["t_starts"], before["t_starts"])
    spec, cand = cand_lists(fld, s)  # (the edited boxes)
    hit = PA.sample_hits(ops, spec, cand, rb.origins, rb.directions, rb.pixel_area, got["ray_indices"], got["t_starts"], got["t_ends"])
    assert int((hit >= 0).sum()) > 50
    op = operator_render(sampler, fld, rb, monkeypatch, **kw)
    for k in ("ray_indices", "t_starts", "t_ends"):
        assert torch.equal(op[k], got[k])
    PA.close([got[k] for k in ("features", "depth", "accumulation", "weights")],
             [op[k] for k in ("features", "depth", "accumulation", "weights")], 1e-5, "edited: fused vs operator route")


def test_render_train_with_boxes_reaches_the_actors(ops):
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler

    s = PA.scene("golden")
    fld = PA.make_actor_field("golden")[0].train()
    fld.hashgrid.config.actor.flip_prob = 0.0
    rb = PA.bundle_of((s["o"], s["d"], s["area"], s["times"]))
    sampler = VolumetricSampler(static_grid("golden")).train()
    torch.manual_seed(0)
    out = sampler.render_train(fld, rb, render_step_size=0.25, near_plane=0.1, far_plane=120.0, actor_boxes=True)
    assert out["weights"].shape == (out["ray_indices"].shape[0], 1) and out["features"].shape == (s["o"].shape[0], 32)
    (out["features"].square().sum() + out["accumulation"].sum() + out["depth"].sum()).backward()
    act = fld.hashgrid.actors
    grads = [gr.hash_table.grad for gr in fld.hashgrid.actor_grids] + [act.actor_positions.grad, act.actor_rotations_6d.grad]
    for g in grads:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_bitwise(ops):
    fld = street_field()
    rays = PA.ragged_rays("street", N_RAGGED, 7)
    o, d, area, times, ts, te, seg = (cuda(a) for a in rays)
    spec, cand = cand_lists(fld, rays)
    fs = fld.field_spec()
    eager = ops.render_fwd_packed_actors(fs, spec, cand, o, d, area, ts, te, seg, return_weights=True)
    torch.cuda.synchronize()  # (the eager call has also made the kernels' one-time occupancy queries)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.render_fwd_packed_actors(fs, spec, cand, o, d, area, ts, te, seg, return_weights=True)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)
