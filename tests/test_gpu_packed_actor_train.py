"""The fused training node for packed samples of a scene with dynamic actors: the packed actor geometry
(nrhip_actor_find_packed), the packed pair positions (nrhip_actor_pair_positions_fwd_packed / _bwd_packed), the packed
training forward with row overrides (nrhip_field_fwd_train_packed_ovr), autograd.NffRenderTrainFn with those overrides behind
NeuRADField.render_train_packed(..., times=...) and VolumetricSampler.render_train(..., fused_actor_training=True).

Scenes, fields, routes and the comparison: tests/packed_actor_train_refs.py on top of tests/packed_actor_refs.py.  Bounds:
bit for bit against the dense kernels on uniform segments; 1e-5 against the numpy oracle and the eval kernel (the bound of
tests/test_gpu_packed_actors.py); node against operator route at the bounds of tests/test_gpu_render_train_packed.py
(2e-5 outputs, 2e-4 gradients, 1e-3 beta)."""
import numpy as np
import pytest
import torch

import packed_actor_refs as PA
import packed_actor_train_refs as TR
import packed_train_refs as T
import synth
from conftest import rel_l2
from gpu_util import cuda, dev, host, to_spec
from gpu_util import ops  # noqa: F401  (fixture)
from neurad_studio_amd import autograd as ag

pytestmark = pytest.mark.gpu

SHAPE_CASES = [(L, F, H, half) for L, F, H in PA.SHAPES for half in (False, True)]
SHAPE_IDS = [f"{L}x{F}-H{H}{'-fp16' if h else ''}" for L, F, H, h in SHAPE_CASES]


def cand_lists(fld, dr):
    return fld.hashgrid.prepare_actors_line(dr[0], dr[1], 0.0, 1.0, dr[3])


# ---- 1. packed geometry against the dense kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("name,S,t_far", [("golden", 37, 16.0), ("street", 21, 108.0)], ids=["golden", "street"])
def test_packed_geometry_is_the_dense_kernels_bit_for_bit(ops, name, S, t_far):
    """Uniform segments: the packed arrays are a dense [R,S] batch.  hits / hit / dirs and the pair positions are
    torch.equal.  The pair backward accumulates with atomics: it is torch.equal where the result cannot depend on their
    order (one or two pairs per launch), and within 1e-4 rel-L2 on all pairs, the bound of tests/test_gpu_actors.py for that
    backward.  Not asserted: torch.equal on all pairs whenever two dense runs happen to repeat -- measured on an MI355X, two
    dense runs on "golden" (69 pairs) repeated bit for bit and the next launch of the same arithmetic still differed in the
    last bits (1.1e-7 rel-L2), and the dense backward did not repeat in the other three cases: repeating twice does not
    make the atomics ordered."""
    R = 48
    rays = TR.uniform_rays(name, R, S, t_far=t_far)
    stats = TR.sample_stats(name, rays)
    print(stats)
    assert stats["pairs"] > 0 and (name != "golden" or stats["overlap"] > 0)
    dr = TR.on_device(rays)
    o, d, area, times, ts, te, seg, ri = dr
    fld = TR.make_train_field(name)[0]
    spec, cand = cand_lists(fld, dr)
    ts2, te2 = ts.view(R, S), te.view(R, S)
    flip_vec = torch.where(torch.arange(R, device="cuda") % 2 == 0, 1.0, -1.0)
    for flip in (None, flip_vec):
        hits_d = ops.actor_hits(spec, cand, o, d, area, ts2, te2)
        dirs_d, hit_d = ops.actor_encode(spec, cand, o, d, area, ts2, te2, torch.zeros((R * S, 32), device="cuda"), flip)
        hits_p, hit_p, dirs_p = ops.actor_find_packed(spec, cand, o, d, area, ts, te, ri, flip)
        assert torch.equal(hits_p, hits_d) and torch.equal(hit_p, hit_d) and torch.equal(dirs_p, dirs_d)
        assert int((hit_p >= 0).sum()) == stats["in_box"] and int((hits_p >= 0).sum()) == stats["pairs"]
        si, ai = ops.actor_pairs(hits_p)
        assert si.shape[0] == stats["pairs"]
        x_d, c_d = ops.actor_pair_positions(spec, o, d, area, ts2, te2, times, si, ai, flip)
        x_p, c_p = ops.actor_pair_positions_packed(spec, o, d, area, ts, te, ri, times, si, ai, flip)
        assert torch.equal(x_p, x_d) and torch.equal(c_p, c_d)
        gx, gc = dev(np.random.default_rng(3).standard_normal((si.shape[0], 3))), dev(np.random.default_rng(4).standard_normal(si.shape[0]))
        dense_bwd = lambda k: ops.actor_pair_positions_bwd(spec, o, d, area, ts2, te2, times, si[k], ai[k], flip, gx[k], gc[k])  # noqa: E731
        packed_bwd = lambda k: ops.actor_pair_positions_packed_bwd(spec, o, d, area, ts, te, ri, times, si[k], ai[k], flip, gx[k], gc[k])  # noqa: E731
        # (a) one pair and two pairs per launch: at most two additions onto a zeroed address, which commute -- the result does
        # not depend on the order of the atomics, so the shared arithmetic must show bit for bit
        multi = (hits_p >= 0).sum(-1)[si] > 1  # pairs of samples in two boxes first
        picks = torch.cat([torch.nonzero(multi)[:4, 0], torch.nonzero(~multi)[:6, 0]])
        assert picks.shape[0] >= 6
        for k in [picks[j:j + 1] for j in range(picks.shape[0])] + [picks[j:j + 2] for j in range(0, picks.shape[0] - 1, 2)]:
            for what, a, b in zip(("d positions", "d rotations_6d"), packed_bwd(k), dense_bwd(k)):
                assert float(b.abs().sum()) > 0 and torch.equal(a, b), (what, k.tolist())
        # (b) every pair: many atomics per address.  Reported: whether two dense runs repeat here; asserted: the bound
        every = torch.arange(si.shape[0], device="cuda")
        b_d, b_d2, b_p = dense_bwd(every), dense_bwd(every), packed_bwd(every)
        repeats = all(torch.equal(a, b) for a, b in zip(b_d, b_d2))
        same = all(torch.equal(a, b) for a, b in zip(b_p, b_d))
        print("flip" if flip is not None else "no flip", "- two dense pair backwards repeat bit for bit:", repeats,
              "- packed equals dense bit for bit:", same)
        for what, a, b in zip(("d positions", "d rotations_6d"), b_p, b_d):
            err = rel_l2(host(a).reshape(-1), host(b).reshape(-1))
            print(what, f"packed vs dense rel-L2 {err:.3e} (bound 1e-4)")
            assert float(b.abs().sum()) > 0 and err < 1e-4, (what, err)


# ---- 2. the forward kernel against the dense override kernel -----------------------------------------------------------
@pytest.mark.parametrize("with_order", [False, True], ids=["batch-order", "ray-order"])
@pytest.mark.parametrize("L,F,H,half", SHAPE_CASES, ids=SHAPE_IDS)
def test_forward_kernel_is_the_dense_override_kernel_bit_for_bit(ops, L, F, H, half, with_order):
    R, S = 23, 37  # two full tiles and five samples per ray, rays not a multiple of the four waves of a workgroup
    rays = TR.uniform_rays("street", R, S)
    o, d, area, times, ts, te, seg, ri = TR.on_device(rays)
    fs = to_spec(ops, PA.shape_params(L, F, H, half), half=half)
    M, LF = R * S, L * F
    rng = np.random.default_rng(5)
    P = 97
    where = rng.permutation(M)[:P]
    where[:3] = (0, S - 1, M - 1)  # a ray's first and last sample, the batch's last
    ovr = np.full(M, -1, np.int32)
    ovr[where] = rng.permutation(P).astype(np.int32)
    dirs = rng.standard_normal((P, 3))
    override = (cuda(ovr), dev(rng.standard_normal((P, LF))), dev(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)))
    order = cuda(rng.permutation(R).astype(np.int32)) if with_order else None
    out_d, saved_d = ops.field_fwd_train(fs, o, d, area, ts.view(R, S), te.view(R, S), order=order, override=override)
    widths = ((32,), (), (), (LF,), (H,), (48,), (2 * H,))
    bufs = [torch.full((M + 1, *w), float("nan"), device="cuda") for w in widths]
    out_p, saved_p = ops.field_fwd_train_packed(fs, o, d, area, ts, te, seg, order=order, out=bufs, override=override)
    names = ("feature", "geo_out", "head", "save_enc", "save_geo_hidden", "save_feat_in", "save_feat_hidden")
    for n, g, w in zip(names, (*out_p, *saved_p), (*out_d, *saved_d)):
        assert bool(torch.isnan(g[M:]).all()), f"{n}: the guard row was written"
        assert bool(torch.isfinite(g[:M]).all()), f"{n}: a live row was not written"
        assert torch.equal(g[:M].reshape(-1), w.reshape(-1)), n
    # save_enc holds the overriding rows
    assert torch.equal(saved_p[0][:M][cuda(where.astype(np.int64))], override[1][cuda(ovr[where].astype(np.int64))])


# ---- 3. the node's forward on ragged segments --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "street"])
def test_ragged_forward_vs_oracle_and_eval_kernel(ops, name):
    rays = PA.ragged_rays(name, 48, 7)
    stats = TR.sample_stats(name, rays)
    print(stats)
    assert stats["pairs"] > 0 and stats["rays_hit"] < 48 and min(np.diff(rays[6])) == 0 and max(np.diff(rays[6])) > 64
    assert (name == "golden") == (stats["overlap"] > 0)
    dr = TR.on_device(rays)
    o, d, area, times, ts, te, seg, ri = dr
    fld, p, ap = TR.make_train_field(name)
    if name == "street":  # every third ray passes no actor: rays without candidates
        assert int((cand_lists(fld, dr)[1][0] == 0).sum()) >= 16
    with torch.no_grad():
        got = TR.node_route(fld, dr)
    PA.close(got, PA.oracle_route(p, ap, rays), 1e-5, f"{name}: node vs oracle,")
    fld.eval()
    with torch.no_grad():
        ev = fld.render_packed(o, d, area, ts, te, segments=seg, times=times, return_weights=True)
    fld.train()
    PA.close(got, ev, 1e-5, f"{name}: node vs eval kernel,")
    # the forward kernel with the node's own overrides: a guard after every per-sample buffer stays untouched
    M, H, LF = ts.shape[0], 32, 32
    ovr = fld._actor_overrides(ag.PackedSamples(ts, te, seg, ri), o, d, area, times)
    assert ovr is not None and int((ovr[0] >= 0).sum()) == stats["in_box"] and ovr[3].shape[0] == stats["pairs"]
    bufs = [torch.full((M + 64, *w), float("nan"), device="cuda") for w in ((32,), (), (), (LF,), (H,), (48,), (2 * H,))]
    with torch.no_grad():
        ops.field_fwd_train_packed(fld.field_spec(), o, d, area, ts, te, seg, out=bufs, override=tuple(t.detach() for t in ovr[:3]))
    for b in bufs:
        assert bool(torch.isfinite(b[:M]).all()) and bool(torch.isnan(b[M:]).all())


# ---- 4. + 5. node against the operator route ---------------------------------------------------------------------------
def both_routes(name, rays, L=8, F=4, H=32, half=False, use_sdf=True, flip_prob=0.0, lg=PA.LG):
    dr = TR.on_device(rays)
    cot = TR.cotangents(rays[0].shape[0], rays[4].shape[0])
    res = {}
    for key, route in (("node", TR.node_route), ("operator", TR.operator_route)):
        fld = TR.make_train_field(name, L, F, H, half, use_sdf, flip_prob, lg)[0]
        assert fld.fused_packed_actors_train_supported() and fld.training
        res[key] = TR.run_route(fld, dr, route, cot)
    return res


NODE_CASES = [("golden", False, True), ("street", False, True), ("street", True, True), ("golden", False, False)]
NODE_IDS = ["golden-overlap", "street", "street-fp16", "golden-density"]


@pytest.mark.parametrize("name,half,use_sdf", NODE_CASES, ids=NODE_IDS)
def test_node_vs_operator_route(ops, name, half, use_sdf):
    """Outputs and every gradient -- static table, the ten MLP parameters, beta, every actor grid's table, actor_positions,
    actor_rotations_6d -- at compare_routes' bounds; flip_prob = 0."""
    rays = PA.ragged_rays(name, 48, 7)
    stats = TR.sample_stats(name, rays)
    assert stats["pairs"] > 0 and (name != "golden" or stats["overlap"] > 0)
    res = both_routes(name, rays, half=half, use_sdf=use_sdf)
    grads = res["node"][1]
    assert ("sdf_to_density.beta" in grads) == use_sdf
    for n in ("hashgrid.actors.actor_positions", "hashgrid.actors.actor_rotations_6d", TR.TABLE):
        assert n in grads and float(grads[n].float().abs().sum()) > 0, n
    assert sum(n.startswith("hashgrid.actor_grids.") for n in grads) == stats["n_actors"] == stats["actors_hit"]
    if half:
        assert grads[TR.TABLE].dtype == torch.float16
    TR.compare_routes(res["node"], res["operator"], f"{name}: ")


def test_untouched_actor_gets_what_the_dense_node_gives_it(ops):
    """Rays that end before most of the cars: an actor no sample touches has the same kind of gradient (None, or zeros) after
    the packed node as after the dense node (render_train) on the same samples."""
    R, S = 6, 21
    rays = TR.uniform_rays("street", R, S, t_far=40.0)
    stats = TR.sample_stats("street", rays)
    print(stats)
    assert 0 < stats["actors_hit"] < stats["n_actors"]
    dr = TR.on_device(rays)
    o, d, area, times, ts, te, seg, ri = dr
    kinds = {}
    for key in ("packed", "dense"):
        fld = TR.make_train_field("street")[0]
        if key == "packed":
            outs = TR.node_route(fld, dr)
        else:
            # the same intervals as a dense batch; the last edge is the sky sample's, far behind every car
            edges = torch.cat([ts.view(R, S), te.view(R, S)[:, -1:], te.view(R, S)[:, -1:] + 1000.0], dim=1)
            outs = fld.render_train(o, d, area, edges, times=times)[:3]
        sum(t.square().sum() for t in outs[:3]).backward()
        kinds[key] = [None if g.hash_table.grad is None else bool((g.hash_table.grad == 0).all())
                      for g in fld.hashgrid.actor_grids]
    print(kinds)
    assert kinds["packed"] == kinds["dense"]
    assert any(k is None or k for k in kinds["packed"]) and any(k is False for k in kinds["packed"])


def test_flip_every_ray_vs_every_sample(ops):
    """flip_prob = 1 in training mode: the node flips every ray, the operator route every sample -- both deterministic, the
    same flips.  (For 0 < p < 1 the two routes draw differently by design: per ray against per sample.)"""
    rays = PA.ragged_rays("street", 48, 7)
    res = both_routes("street", rays, flip_prob=1.0)
    TR.compare_routes(res["node"], res["operator"], "flip: ")
    plain = both_routes("street", rays)["node"]
    assert not torch.equal(plain[0][0], res["node"][0][0])  # the flip changes what the in-box samples read


# ---- 6. no pairs: the static node --------------------------------------------------------------------------------------
STATIC_NAMES = [TR.TABLE, "sdf_to_density.beta"] + [f"mlp_{m}.layers.{k}.{w}" for m, n in (("geo", 2), ("feature", 3))
                                                    for k in range(n) for w in ("weight", "bias")]


def test_without_pairs_the_call_is_the_static_node(ops):
    """"street" rays [::3], none with a candidate: outputs and the static-table / MLP / beta gradients are those of the same
    field built without actors, bit for bit.  M >= ops._BINNED_MIN_SAMPLES, so that the static node's own table gradient is
    bit-reproducible (the partition; below that size it is an atomic scatter, which does not repeat even against itself)."""
    R = 100
    rays = TR.subset_rays("street", 0, 3, R, 7, counts=(330,) * R)
    assert TR.sample_stats("street", rays)["pairs"] == 0 and rays[4].shape[0] >= ops._BINNED_MIN_SAMPLES
    dr = TR.on_device(rays)
    fld = TR.make_train_field("street")[0]
    assert int((cand_lists(fld, dr)[1][0] > 0).sum()) == 0  # no ray has a candidate
    cot = TR.cotangents(R, rays[4].shape[0])
    got = TR.run_route(fld, dr, TR.node_route, cot)
    twin = TR.make_static_twin()
    want = TR.run_route(twin, dr, lambda f, r: f.render_train_packed(r[0], r[1], r[2], r[4], r[5], segments=r[6]), cot)
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    differ = [n for n in STATIC_NAMES if not torch.equal(got[1][n], want[1][n])]
    assert not differ, differ
    assert not any(n.startswith("hashgrid.actor") for n in got[1])  # the actor branch was not entered


@pytest.mark.parametrize("counts", [(0,) * 7, (), (0, 0, 0, 19, 0, 0)], ids=["M=0", "R=0", "one-segment"])
def test_degenerate_batches(ops, counts):
    R = len(counts)
    rays = TR.subset_rays("street", 1, 3, R, 5, counts=counts)  # (rays that do pass the cars)
    dr = TR.on_device(rays)
    fld = TR.make_train_field("street")[0]
    outs = TR.node_route(fld, dr)
    M = sum(counts)
    assert [tuple(t.shape) for t in outs] == [(R, 32), (R, 1), (R, 1), (M,)]
    sum(t.sum() for t in outs).backward()
    if M == 0:
        assert all(bool((t == 0).all()) for t in outs)
        for n, p in fld.named_parameters():
            assert p.grad is None or bool((p.grad == 0).all()), n
    else:
        empty = torch.from_numpy(np.asarray(counts) == 0).cuda()
        assert all(bool((t[empty] == 0).all()) for t in outs[:3]) and bool((outs[2][~empty] > 0).all())
        want = TR.operator_route(TR.make_train_field("street")[0], dr)
        PA.close(outs, want, 2e-5, "one segment: node vs operator,")
        assert bool(torch.isfinite(fld.hashgrid.static_grid.hash_table.grad).all())


# ---- 7. the partition source -------------------------------------------------------------------------------------------
def test_partition_source_with_overridden_rows_zeroed(ops):
    """M = 33 110 >= ops._BINNED_MIN_SAMPLES: the packed radix partition forms the static table's gradient from dL/d enc with
    the overridden rows zeroed.  A 2^17-row static table (instead of 2^11) so that rows exist that only in-box samples
    touch: there the gradient must be exactly zero."""
    lg = 17
    rays = PA.ragged_rays("street", 301, 7, counts=(110,) * 301)
    M = rays[4].shape[0]
    assert M >= ops._BINNED_MIN_SAMPLES
    stats = TR.sample_stats("street", rays)
    assert stats["in_box"] > 1000
    res = both_routes("street", rays, lg=lg)
    TR.compare_routes(res["node"], res["operator"], "partition: ")
    # rows of the static table by who touches them: the table gradient of all-ones dL/d enc from either set of samples
    dr = TR.on_device(rays)
    o, d, area, times, ts, te, seg, ri = dr
    fld = TR.make_train_field("street", lg=lg)[0]
    spec, cand = cand_lists(fld, dr)
    hit = ops.actor_find_packed(spec, cand, o, d, area, ts, te, ri)[1] >= 0
    assert int(hit.sum()) == stats["in_box"]
    g = fld.hashgrid.static_grid
    touched = {}
    for key, m in (("in", hit), ("out", ~hit)):
        ones = torch.ones((int(m.sum()), g.spec.out_dim), device="cuda")
        gt = ops.encode_bwd(g.spec, fld.hashgrid.static_scale, o[ri[m]], d[ri[m]], area[ri[m]], ts[m][:, None], te[m][:, None], ones)
        touched[key] = (gt != 0).any(-1)
    only_in = touched["in"] & ~touched["out"]
    print("static rows touched by in-box samples only:", int(only_in.sum()), "of", int(touched["in"].sum()))
    assert int(only_in.sum()) > 0
    node_grad = res["node"][1][TR.TABLE]
    assert bool((node_grad[only_in] == 0).all())
    assert float(node_grad[touched["out"]].abs().sum()) > 0


# ---- 8. the sampler ----------------------------------------------------------------------------------------------------
def test_sampler_hands_the_candidate_lists_to_the_node(ops, monkeypatch):
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler

    s = PA.scene("golden")
    rb = PA.bundle_of((s["o"], s["d"], s["area"], s["times"]))
    sampler = VolumetricSampler(TR.static_grid("golden")).train()
    kw = dict(render_step_size=0.25, near_plane=0.1, far_plane=120.0, actor_boxes=True)
    keys = ("features", "depth", "accumulation", "weights")

    def run(fused_training=True, refuse=False, **extra):
        fld = TR.make_train_field("golden")[0]
        fld.fused_training = fused_training
        calls = []
        real = type(fld).render_train_packed
        with monkeypatch.context() as m:
            m.setattr(type(fld), "render_train_packed", lambda self, *a, **k: calls.append(k) or real(self, *a, **k))
            if refuse:
                m.setattr(type(fld), "fused_packed_actors_train_supported", lambda self: False)
            torch.manual_seed(0)
            out = sampler.render_train(fld, rb, **kw, **extra)
        (out["features"].square().sum() + out["accumulation"].sum() + out["depth"].sum() + out["weights"].square().sum()).backward()
        return out, TR.field_grads(fld), calls

    default, fused = run(), run(fused_actor_training=True)
    assert default[2] == [] and len(fused[2]) == 1 and fused[2][0]["actor_cand"] is not None  # the march's own lists
    for k in ("ray_indices", "t_starts", "t_ends"):
        assert torch.equal(default[0][k], fused[0][k])
    assert set(default[0]) == set(fused[0]) and all(default[0][k].shape == fused[0][k].shape for k in default[0])
    M = fused[0]["t_starts"].shape[0]
    assert M > 100 and fused[0]["weights"].shape == (M, 1)
    act = ["hashgrid.actors.actor_positions", "hashgrid.actors.actor_rotations_6d"] + \
        [n for n in fused[1] if n.startswith("hashgrid.actor_grids.")]
    assert len(act) == 5
    for n in act:
        g = fused[1][n]
        assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0, n
    TR.compare_routes(([fused[0][k] for k in keys], fused[1]), ([default[0][k] for k in keys], default[1]), "sampler: ")
    # fused_training off, or a field the gate refuses: silently the operator route, same keys
    for fallback in (run(fused_training=False, fused_actor_training=True), run(refuse=True, fused_actor_training=True)):
        assert fallback[2] == [] and set(fallback[0]) == set(default[0])
        for k in default[0]:
            assert torch.equal(fallback[0][k], default[0][k]), k


# ---- 9. determinism ----------------------------------------------------------------------------------------------------
def test_forward_and_static_table_gradient_repeat_bit_for_bit(ops):
    """With `order` given, two runs give the same outputs and the same static-table gradient bit for bit: the forward and
    the table gradient's partition use no atomics (M >= ops._BINNED_MIN_SAMPLES).  Not asserted bitwise: actor_positions,
    actor_rotations_6d and the actor grids' tables -- the pair backward and the multi-grid scatter accumulate with atomics,
    whose order varies between runs -- nor what depends on them."""
    rays = PA.ragged_rays("street", 301, 7, counts=(110,) * 301)
    assert rays[4].shape[0] >= ops._BINNED_MIN_SAMPLES
    dr = TR.on_device(rays)
    cot = TR.cotangents(301, rays[4].shape[0])
    runs = []
    for _ in range(2):
        fld = TR.make_train_field("street")[0]
        fld.order_rays = True
        runs.append(TR.run_route(fld, dr, TR.node_route, cot))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1][TR.TABLE], runs[1][1][TR.TABLE])


# ---- 10. under autocast ------------------------------------------------------------------------------------------------
def _render_call(case):
    """-> (the field, its extra parameters by name, call() -> the node's four outputs) of one of the three render nodes"""
    kind, _, head = case.partition("-")
    if kind == "dense":  # render_train with a temporal appearance embedding, one block of embedding rows per ray
        R, S, A, n_per, duration = 23, 17, 8, 4, 8.0
        fld = T.make_field(8, 4, 32, head == "sdf")[0]
        o, d, area, ts, te, _, _ = T.on_device(T.packed_rays((S,) * R, 7))
        edges = torch.cat([ts.view(R, S), te.view(R, S)[:, -1:]], dim=1)  # (the last sample's far edge is the sky distance)
        emb = dev(synth.normal((R * n_per, A), 5)).requires_grad_(True)
        appearance = (emb, torch.arange(R, device="cuda")[:, None], dev(synth.uniform((R, 1), 0.0, duration, 6)),
                      (duration, n_per, True))
        return fld, {"appearance_embedding": emb}, lambda: fld.render_train(o, d, area, edges, appearance)
    if kind == "packed":
        fld = T.make_field(8, 4, 32, head == "sdf")[0]
        o, d, area, ts, te, seg, _ = T.on_device(T.packed_rays(T.RAGGED, 7))
        return fld, {}, lambda: fld.render_train_packed(o, d, area, ts, te, segments=seg)
    fld = TR.make_train_field("golden")[0]  # flip_prob = 0
    dr = TR.on_device(PA.ragged_rays("golden", 48, 7))
    return fld, {}, lambda: TR.node_route(fld, dr)


ATOMIC = ("hashgrid.actors.actor_positions", "hashgrid.actors.actor_rotations_6d")


@pytest.mark.parametrize("case", ["dense-sdf", "dense-density", "packed-sdf", "packed-density", "actors"])
def test_render_nodes_under_autocast_are_the_plain_run(ops, monkeypatch, case):
    """The trainer runs under autocast, and custom_fwd(cast_inputs=float32) walks the node's arguments: every tensor of the
    sample layout has to be an argument of its own (a tuple subclass holding them cannot be rebuilt by the cast).  The same
    fp32 inputs plainly and inside torch.autocast("cuda", float16), backward each time: outputs and parameter gradients are
    torch.equal.  What makes that possible: the table gradients -- static table and actor grids -- come from the partition
    (ops._BINNED_MIN_SAMPLES = 1: no float atomics), and a cell of the embedding's gradient receives at most two additions
    onto zero (one block of rows per ray), which commute.  The exception are the trajectories, whose gradient the pair
    backward accumulates with float atomics in an order that varies: compare_routes' bound for a parameter gradient."""
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    runs = []
    for cast in (False, True):
        fld, extra, call = _render_call(case)
        with torch.autocast("cuda", dtype=torch.float16, enabled=cast):
            outs = call()
        assert all(t.dtype == torch.float32 for t in outs)
        sum((t * dev(synth.normal(tuple(t.shape), 81 + k))).sum() for k, t in enumerate(outs)).backward()
        grads = {**TR.field_grads(fld), **{n: t.grad.detach().clone() for n, t in extra.items()}}
        runs.append(([t.detach() for t in outs], grads))
    (out_p, grad_p), (out_c, grad_c) = runs
    assert all(torch.equal(a, b) for a, b in zip(out_p, out_c))
    assert set(grad_p) == set(grad_c) and TR.TABLE in grad_p and set(extra) <= set(grad_p)
    assert (case == "actors") == all(n in grad_p for n in ATOMIC)
    for n in grad_p:
        assert float(grad_p[n].abs().sum()) > 0, n
        if n in ATOMIC:
            err = rel_l2(host(grad_p[n]).reshape(-1), host(grad_c[n]).reshape(-1))
            print(f"d {n}: autocast vs plain rel-L2 {err:.3e} (bound 2e-4)")
            assert err < 2e-4, (n, err)
        else:
            assert torch.equal(grad_p[n], grad_c[n]), n
