"""dL/d(origins, directions) through the pair positions of PACKED samples: the kernel (nrhip_actor_pair_positions_bwd_rays_packed
/ ops.actor_pair_positions_packed_bwd_rays), the node that calls it (NeuRADField.render_train_packed(..., times=...,
actor_ray_gradients=True) with rays that require grad) and the sampler's opt-in (VolumetricSampler.render_train(...,
fused_actor_ray_gradients=True)).

Scenes, pairs and references: tests/packed_actor_ray_grad_refs.py on top of tests/actor_refs.py (kernel) and
tests/packed_actor_train_refs.py (node, sampler).  Bounds: actor_refs.pair_grad_bound with dpp = log2 G against float64;
bit for bit on the designed scene whose sums are exact, between runs, under a permutation of the rays and in a graph; the
node's ray gradient is the fp32 sum of the two kernels' outputs bit for bit (two terms: the sum commutes); node against
operator route at compare_routes' bounds, ray gradients per ray under the 1e-3 median guard of
tests/test_gpu_packed_ray_grads.py::test_sampler_opt_in_vs_the_fallback."""
import functools

import numpy as np
import pytest
import torch

import actor_refs as AR
import packed_actor_ray_grad_refs as RG
import packed_actor_refs as PA
import packed_actor_train_refs as TR
import packed_restatement as PR
import synth
from conftest import rel_l2
from gpu_util import cuda, host
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NAME = "nrhip_actor_pair_positions_bwd_rays_packed"


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def make_spec(ops, a):
    """ops.ActorSpec from a scene's arrays; the pair kernels never read the tables: one small table for all"""
    A = a["positions"].shape[1]
    table = cuda(synth.hash_table(4 * 2**9, 2, seed=900, scale=0.7))
    return ops.ActorSpec(cuda(a["timestamps"]), cuda(a["positions"]), cuda(a["rotations_6d"]), cuda(a["present"]),
                         cuda(a["bounds"]), ops.GridSpec(4, 2, 9, 64, 1024), [table] * A, actor_scale=a["scale"])


def run_kernel(ops, actors, rays, pairs, lanes=0, fill=None):
    """the kernel on host arrays -> fp32 arrays (grad_origins, grad_directions).  rays: (o, d, area, times, ts, te, seg,
    flip | None), pairs: (si, ai, gx, gs).  fill: the entry point is called on the caller's own buffers, pre-filled with `fill`
    (the wrapper allocates its outputs itself)"""
    o, d, area, times, ts, te, seg, flip = rays
    si, ai, gx, gs = pairs
    spec = make_spec(ops, actors)
    args = tuple(cuda(np.asarray(x, f32)) for x in (o, d, area, ts, te)) + (cuda(seg),)
    t, fl = cuda(times), None if flip is None else cuda(flip)
    dsi, dai, dgx, dgs = cuda(si), cuda(ai), cuda(gx), cuda(gs)
    if fill is None:
        go, gd = ops.actor_pair_positions_packed_bwd_rays(spec, *args, t, dsi, dai, fl, dgx, dgs, lanes_per_ray=lanes)
    else:
        a, keep_a = spec.c_actors()
        r, keep_r = ops._c_packed_rays("test", *args)
        go, gd = (torch.full((len(seg) - 1, 3), fill, device="cuda") for _ in range(2))
        ops.launch(NAME, a, r, t, dsi, dai, fl, len(si), dgx, dgs, lanes, go, gd)
    return host(go), host(gd)


GENERIC = {"mag<1": (dict(seed=2), False), "mag>1": (dict(seed=2, scale=1.5), True), "wide": (dict(seed=1, wide=True), False)}


@functools.lru_cache(maxsize=None)
def generic_case(name, ragged, with_flip):
    """-> scene, packed rays, the surviving pairs with their cotangents, the float64 reference; shared by the group sizes"""
    kw, random_pairs = GENERIC[name]
    sc = AR.generic_scene(**kw)
    R = sc["o"].shape[0]
    si, ai = RG.random_sorted_pairs(sc) if random_pairs else RG.production_pairs(sc)
    rays, keep, psi = RG.cut(sc, si, ai, RG.cut_counts(R) if ragged else None)
    flip = np.where(np.arange(R) % 3 == 1, -1.0, 1.0).astype(f32) if with_flip else None
    ref = AR.pair_case(sc, si[keep], ai[keep], flip, 60 + len(psi))
    return sc, (*rays, flip), (psi, ai[keep], ref["gx"], ref["gs"]), ref


def worst_over_bound(go, gd, ref, dpp, rows=None):
    worst = 0.0
    for key, got in (("go", go), ("gd", gd)):
        bound, n = AR.pair_grad_bound(ref, key, dpp=dpp)
        rows_ = np.ones(len(got), bool) if rows is None else rows
        assert (got[rows_ & (n[:, 0] == 0)] == 0).all(), (key, "a ray without pairs")
        worst = max(worst, float((np.abs(got.astype(f64) - ref[key]) / np.maximum(bound, 1e-300))[rows_].max()))
    return worst


# ---- 1. against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_flip", [False, True], ids=["no-flip", "flip"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name", list(GENERIC))
def test_per_element_against_float64(ops, name, ragged, with_flip):
    """the scene's production pairs (mag>1: random pairs, the contracted branch) on uniform segments and on a ragged cut (a
    per-ray prefix, rays without samples among them), every group size; NaN-filled buffers: every row is WRITTEN"""
    sc, rays, pairs, ref = generic_case(name, ragged, with_flip)
    P, R = len(pairs[0]), sc["o"].shape[0]
    assert P >= 200 and (ref["n_ray"] > 0).sum() >= 30
    if name == "mag>1":
        assert ref["outside"].sum() > P // 2  # the contracted branch
    for lanes in RG.LANES:
        go, gd = run_kernel(ops, sc, rays, pairs, lanes, fill=float("nan"))
        assert np.isfinite(go).all() and np.isfinite(gd).all(), (lanes, "a row was not written, or is not finite")
        assert np.abs(go).sum() > 0 and np.abs(gd).sum() > 0
        worst = worst_over_bound(go, gd, ref, RG.log2_group(lanes, P, R))
        print(f"{name} {'ragged' if ragged else 'uniform'} flip={with_flip} lanes {lanes} P {P}: worst err / bound {worst:.3f}")
        assert worst <= 1.0, (lanes, worst)
        a = run_kernel(ops, sc, rays, pairs, lanes)  # the wrapper (its own buffers) returns the same bits
        assert np.array_equal(a[0], go) and np.array_equal(a[1], gd)


# ---- 2. exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", RG.LANES)
def test_exact_sums_at_the_groups_boundaries(ops, lanes):
    """Every contribution is a dyadic number (packed_actor_ray_grad_refs.exact_case): the sums are exact in any order, so the
    kernel equals the float64 value bit for bit -- a dropped or doubled pair shows.  Pairs per ray: 0, 1, G - 1, G, G + 1,
    2 G + 1, 190, two on one sample; rays without samples between rays with pairs; the first pair is the list's first, the
    last its last.  Rays without pairs read exactly 0.0 over the NaNs the buffers held."""
    for G in ((16, 32, 64) if lanes == 0 else (lanes,)):
        c = RG.exact_case(G)
        go, gd = run_kernel(ops, c["actors"], c["rays"], c["pairs"], lanes, fill=float("nan"))
        for key, got in (("go", go), ("gd", gd)):
            assert np.array_equal(AR.bits(got), AR.bits(c[key].astype(f32))), (G, key, got, c[key])
            assert (got[c["n_pairs"] == 0] == 0).all() and (np.abs(got[c["n_pairs"] > 0]).sum(-1) > 0).all()


# ---- 3. bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", RG.LANES)
def test_reproducible_and_independent_of_the_rays_place(ops, lanes):
    sc, rays, pairs, _ = generic_case("wide", True, True)
    a = run_kernel(ops, sc, rays, pairs, lanes)
    b = run_kernel(ops, sc, rays, pairs, lanes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # no atomics: the same bits
    R = sc["o"].shape[0]
    perm = np.random.default_rng(5).permutation(R)
    assert (perm != np.arange(R)).sum() > R // 2
    rays_p, pairs_p, _ = RG.take_rays(rays, pairs, perm)
    c = run_kernel(ops, sc, rays_p, pairs_p, lanes)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm])
    if lanes:  # every other ray removed, the same forced group size: the rays that stay keep their bits
        stay = np.arange(1, R, 2)
        rays_h, pairs_h, _ = RG.take_rays(rays, pairs, stay)
        assert 0 < len(pairs_h[0]) < len(pairs[0])
        h = run_kernel(ops, sc, rays_h, pairs_h, lanes)
        assert np.array_equal(h[0], a[0][stay]) and np.array_equal(h[1], a[1][stay])


def test_no_pairs_zeroes_the_outputs(ops):
    sc, rays, pairs, _ = generic_case("mag<1", True, False)
    none = tuple(x[:0] for x in pairs)
    for lanes in RG.LANES:
        go, gd = run_kernel(ops, sc, rays, none, lanes, fill=float("nan"))
        assert go.shape == (sc["o"].shape[0], 3) and (go == 0).all() and (gd == 0).all()
    # a batch without samples, and one without rays
    o, d, area, times = rays[:4]
    e = np.zeros((0,), f32)
    go, gd = run_kernel(ops, sc, (o, d, area, times, e, e, np.zeros(len(o) + 1, np.int64), None), none, fill=float("nan"))
    assert (go == 0).all() and (gd == 0).all()
    go, gd = run_kernel(ops, sc, (o[:0], d[:0], area[:0], times[:0], e, e, np.zeros(1, np.int64), None), none)
    assert go.shape == (0, 3) and gd.shape == (0, 3)


@pytest.mark.parametrize("lanes", [16, 64, 0])
def test_non_finite_row_stays_in_its_ray(ops, lanes):
    """a NaN or inf in one pair's grad_x01 makes that ray's gradient non-finite and leaves every other ray in its bound"""
    sc, rays, pairs, ref = generic_case("mag<1", False, False)
    si, ai, gx, gs = pairs
    S, R = sc["starts"].shape[1], sc["o"].shape[0]
    ray_of_pair = si // S
    per = np.bincount(ray_of_pair, minlength=R)
    for bad, ray in ((np.nan, int(per.argmax())), (np.inf, int(np.nonzero(per == per[per > 0].min())[0][0]))):
        gb = gx.copy()
        gb[np.nonzero(ray_of_pair == ray)[0][per[ray] // 2], 1] = bad
        go, gd = run_kernel(ops, sc, rays, (si, ai, gb, gs), lanes)
        others = np.arange(R) != ray
        assert not np.isfinite(go[ray]).all() and not np.isfinite(gd[ray]).all()
        assert np.isfinite(go[others]).all() and np.isfinite(gd[others]).all()
        assert worst_over_bound(go, gd, ref, RG.log2_group(lanes, len(si), R), rows=others) <= 1.0


# ---- 4. graph replay -----------------------------------------------------------------------------------------------------
def test_replays_in_a_graph(ops):
    sc, rays, pairs, _ = generic_case("wide", True, True)
    o, d, area, times, ts, te, seg, flip = rays
    spec = make_spec(ops, sc)
    args = tuple(cuda(np.asarray(x, f32)) for x in (o, d, area, ts, te)) + (cuda(seg), cuda(times))
    tail = (cuda(pairs[0]), cuda(pairs[1]), cuda(flip), cuda(pairs[2]), cuda(pairs[3]))
    step = lambda: ops.actor_pair_positions_packed_bwd_rays(spec, *args, *tail)  # noqa: E731
    eager = [t.clone() for t in step()]
    assert float(eager[0].abs().sum()) > 0 and float(eager[1].abs().sum()) > 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


# ---- 5. the node ---------------------------------------------------------------------------------------------------------
ATOMIC = ("hashgrid.actors.actor_positions", "hashgrid.actors.actor_rotations_6d")


def node_step(fld, dr, cot, need_o, need_d, flag=None):
    o, d = dr[0].clone().requires_grad_(need_o), dr[1].clone().requires_grad_(need_d)
    flag = (need_o or need_d) if flag is None else flag
    outs = fld.render_train_packed(o, d, dr[2], dr[4], dr[5], segments=dr[6], times=dr[3], actor_ray_gradients=flag)
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    return [t.detach() for t in outs], TR.field_grads(fld), o.grad, d.grad


def spy_on(monkeypatch, ops):
    """record the outputs of the two ray-gradient ops: the static encoding's and the pair positions'"""
    calls = {"static": [], "actor": []}
    real_s, real_a = ops.encode_bwd_rays_packed, ops.actor_pair_positions_packed_bwd_rays

    def spy_s(*a, **k):
        out = real_s(*a, **k)
        calls["static"].append((out[0].clone(), out[1].clone()))
        return out

    def spy_a(*a, **k):
        out = real_a(*a, **k)
        calls["actor"].append((out[0].clone(), out[1].clone()))
        return out

    monkeypatch.setattr(ops, "encode_bwd_rays_packed", spy_s)
    monkeypatch.setattr(ops, "actor_pair_positions_packed_bwd_rays", spy_a)
    return calls


@pytest.mark.parametrize("name,half", [("golden", False), ("street", False), ("street", True)],
                         ids=["golden-overlap", "street", "street-fp16"])
def test_node_returns_the_sum_of_the_two_kernels_gradients(ops, monkeypatch, name, half):
    """(8, 4, 32), fp32 and fp16 storage, flip_prob = 0.  o.grad / d.grad are the fp32 sum of the static op's and the actor
    op's rows bit for bit (two terms: either order gives the same bits).  ops._BINNED_MIN_SAMPLES = 1 puts the table
    gradients -- static table, actor grids -- on the partition, which is deterministic: outputs and those gradients equal the
    same call with fixed rays bit for bit; the trajectories' gradient accumulates with float atomics: 1e-6 rel-L2."""
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    rays = PA.ragged_rays(name, 48, 7)
    stats = TR.sample_stats(name, rays)
    assert stats["pairs"] > 0
    dr = TR.on_device(rays)
    R, M = rays[0].shape[0], rays[4].shape[0]
    cot = TR.cotangents(R, M)
    calls = spy_on(monkeypatch, ops)
    fld = TR.make_train_field(name, 8, 4, 32, half)[0]
    outs, grads, go, gd = node_step(fld, dr, cot, True, True)
    assert len(calls["static"]) == 1 and len(calls["actor"]) == 1
    (so, sd), (ao, ad) = calls["static"][0], calls["actor"][0]
    assert go.shape == (R, 3) and torch.equal(go, so + ao) and torch.equal(gd, sd + ad)
    for t in (so, sd, ao, ad):
        assert bool(torch.isfinite(t).all()) and float(t.abs().sum()) > 0
    assert int((ao.abs().sum(-1) > 0).sum()) == stats["rays_hit"]  # exactly the rays with in-box samples
    empty = torch.from_numpy(np.diff(rays[6]) == 0).cuda()
    assert bool((go[empty] == 0).all()) and bool((gd[empty] == 0).all())
    # the same step with fixed rays: the same outputs and parameter gradients, no ray-gradient launch
    fld2 = TR.make_train_field(name, 8, 4, 32, half)[0]
    outs2, grads2, go2, gd2 = node_step(fld2, dr, cot, False, False, flag=True)  # (with fixed rays the flag changes nothing)
    assert len(calls["static"]) == 1 and len(calls["actor"]) == 1 and go2 is None and gd2 is None
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    assert set(grads) == set(grads2) and all(n in grads for n in ATOMIC)
    for n in grads:
        if n in ATOMIC:
            err = rel_l2(host(grads[n]).reshape(-1), host(grads2[n]).reshape(-1))
            print(f"d {n}: moving vs fixed rays rel-L2 {err:.3e} (bound 1e-6)")
            assert err < 1e-6, (n, err)
        else:
            assert torch.equal(grads[n], grads2[n]), n
    # only one of the two requires grad: only that gradient, the same bits
    for which in (0, 1):
        f3 = TR.make_train_field(name, 8, 4, 32, half)[0]
        _, _, go3, gd3 = node_step(f3, dr, cot, which == 0, which == 1)
        assert (go3 is None) == (which == 1) and (gd3 is None) == (which == 0)
        assert torch.equal(go3, go) if which == 0 else torch.equal(gd3, gd)


def test_without_require_actor_grad_the_ray_gradient_is_the_static_share(ops, monkeypatch):
    """the reference's no_grad around _split_static_vs_actors: without require_actor_grad the actor branch hands the rays
    nothing, on packed samples as on dense ones"""
    rays = PA.ragged_rays("street", 48, 7)
    dr = TR.on_device(rays)
    cot = TR.cotangents(rays[0].shape[0], rays[4].shape[0])
    calls = spy_on(monkeypatch, ops)
    fld = TR.make_train_field("street")[0]
    fld.hashgrid.config.require_actor_grad = False
    _, grads, go, gd = node_step(fld, dr, cot, True, True)
    assert len(calls["static"]) == 1 and calls["actor"] == []
    assert torch.equal(go, calls["static"][0][0]) and torch.equal(gd, calls["static"][0][1])
    assert not any(n in grads for n in ATOMIC)


# ---- 6. node against the operator route with the same moving rays ----------------------------------------------------------
def per_ray_distance(what, node, operator, live):
    """rays without samples: exactly 0 on both routes; the others: relative distance per ray, printed, median < 1e-3"""
    a, c = host(node).astype(f64), host(operator).astype(f64)
    assert (a[~live] == 0).all() and (c[~live] == 0).all()
    per_ray = np.linalg.norm(a[live] - c[live], axis=-1) / np.linalg.norm(c[live], axis=-1)
    print(f"d {what}: node vs operator route per ray: median {np.median(per_ray):.3e}, worst {per_ray.max():.3e}")
    assert np.median(per_ray) < 1e-3, (what, np.sort(per_ray)[-5:])


@pytest.mark.parametrize("name,half", [("golden", False), ("street", False), ("street", True)],
                         ids=["golden-overlap", "street", "street-fp16"])
def test_node_vs_operator_route_with_moving_rays(ops, name, half):
    rays = PA.ragged_rays(name, 48, 7)
    stats = TR.sample_stats(name, rays)
    live = np.diff(rays[6]) > 0
    assert stats["rays_hit"] * 5 >= live.sum()  # at least a fifth of the compared rays have in-box samples
    dr = TR.on_device(rays)
    cot = TR.cotangents(rays[0].shape[0], rays[4].shape[0])
    fld = TR.make_train_field(name, 8, 4, 32, half)[0]
    node = node_step(fld, dr, cot, True, True)
    fld2 = TR.make_train_field(name, 8, 4, 32, half)[0]
    o, d = dr[0].clone().requires_grad_(True), dr[1].clone().requires_grad_(True)
    op = TR.run_route(fld2, (o, d, *dr[2:]), TR.operator_route, cot)
    TR.compare_routes(node[:2], op, f"{name} moving rays: ")
    # (measured on an MI355X, origins / directions: golden median 2.0e-7 / 2.4e-7, worst ray 9.2e-7; street 1.5e-7 / 1.7e-7,
    #  worst 5.4e-7; street fp16 storage 1.9e-7 / 1.9e-7, worst 1.2e-6; the sampler test below 1.8e-7 / 1.5e-7, worst 5.6e-7)
    per_ray_distance("origins", node[2], o.grad, live)
    per_ray_distance("directions", node[3], d.grad, live)


# ---- 7. the sampler ------------------------------------------------------------------------------------------------------
def test_sampler_opt_in_keeps_moving_rays_on_the_node(ops, monkeypatch):
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler

    s = PA.scene("golden")
    sampler = VolumetricSampler(TR.static_grid("golden")).train()
    kw = dict(render_step_size=0.25, near_plane=0.1, far_plane=120.0, actor_boxes=True)
    keys = ("features", "depth", "accumulation", "weights")
    R = s["o"].shape[0]

    def refuse(*a, **k):
        raise AssertionError("the wrong route ran")

    def moving_bundle():
        rb = PA.bundle_of((s["o"], s["d"], s["area"], s["times"]))
        rb.origins.requires_grad_(True), rb.directions.requires_grad_(True)
        return rb

    # every opt-in on: the node, which reads the bundle's own tensors (no gather of the ray constants)
    fld, rb = TR.make_train_field("golden")[0], moving_bundle()
    calls = []
    real = type(fld).render_train_packed
    with monkeypatch.context() as m:
        m.setattr(VolumetricSampler, "_gather", staticmethod(refuse))
        m.setattr(type(fld), "render_train_packed", lambda self, *a, **k: calls.append(k) or real(self, *a, **k))
        torch.manual_seed(0)
        got = sampler.render_train(fld, rb, fused_actor_training=True, fused_actor_ray_gradients=True, **kw)
    assert len(calls) == 1 and calls[0]["actor_ray_gradients"] is True and calls[0]["actor_cand"] is not None
    ri, ts, te = got["ray_indices"], got["t_starts"], got["t_ends"]
    M = ri.shape[0]
    assert M > 100 and got["weights"].shape == (M, 1)
    cot = TR.cotangents(R, M, 91)
    outs = [got[k] for k in keys]
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    fused = ([t.detach().reshape(c.shape) for t, c in zip(outs, cot)], TR.field_grads(fld))
    # the operator route fed the RETURNED samples (the stratified draw is shared), the same moving rays
    fld2, rb2 = TR.make_train_field("golden")[0], moving_bundle()
    seg = PR.segments_from_counts(np.bincount(host(ri), minlength=R))
    dr2 = (rb2.origins, rb2.directions, rb2.pixel_area.reshape(-1), rb2.times.reshape(-1), ts, te, cuda(seg), ri)
    op = TR.run_route(fld2, dr2, TR.operator_route, cot)
    TR.compare_routes(fused, op, "sampler, moving rays: ")
    live = np.diff(seg) > 0
    per_ray_distance("origins", rb.origins.grad, rb2.origins.grad, live)
    per_ray_distance("directions", rb.directions.grad, rb2.directions.grad, live)
    # without fused_actor_ray_gradients the same call takes the operator route, bit for bit what no opt-in at all gives
    runs = []
    for extra in ({"fused_actor_training": True}, {}, {"fused_actor_training": True, "fused_ray_gradients": True}):
        f3, rb3 = TR.make_train_field("golden")[0], moving_bundle()
        with monkeypatch.context() as m:
            m.setattr(type(f3), "render_train_packed", refuse)
            torch.manual_seed(0)
            runs.append(sampler.render_train(f3, rb3, **kw, **extra))
    for other in runs[1:]:
        assert set(other) == set(runs[0]) == set(got)
        for k in runs[0]:
            assert torch.equal(other[k], runs[0][k]), k
    # fixed rays: the flag changes nothing (no ray gradient is asked for)
    f4 = TR.make_train_field("golden")[0]
    rb4 = PA.bundle_of((s["o"], s["d"], s["area"], s["times"]))
    with monkeypatch.context() as m:
        m.setattr(ops, "actor_pair_positions_packed_bwd_rays", refuse)
        m.setattr(ops, "encode_bwd_rays_packed", refuse)
        torch.manual_seed(0)
        out4 = sampler.render_train(f4, rb4, fused_actor_training=True, fused_actor_ray_gradients=True, **kw)
        (out4["features"].sum() + out4["depth"].sum()).backward()
    assert rb4.origins.grad is None and torch.equal(out4["t_starts"], ts)
