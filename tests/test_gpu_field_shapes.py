"""The fused field kernels on grids with L * F < 32 (BASELINE config[0]'s 1 x 4, NeuRAD tiny's 4 x 2, and 4 x 4 / 8 x 2):
the padded encoding frame of render.hip against the numpy oracle, the reference's own outputs and gradients
(tests/golden/field_tiny.npz, field_neurad_tiny.npz, field_neurad_tiny_actors.npz) and the operator-level path."""
import numpy as np
import pytest
import torch

import neurad_oracle as O
import synth
from conftest import load_golden, rel_l2
from builders import SHAPES, actor_params, field_params, sample_rays, shape_params, tagged_field_params, trajectories
from gpu_util import TIGHT, TOL, actor_rays, bundle, dev, host, load_field_weights, to_spec, torch_sdf_render
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SMALL = [(1, 4), (4, 2), (4, 4), (8, 2)]  # (L, F) of the padded-frame instantiations


# ---- 1. the kernels against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("LF", SMALL, ids=[f"L{L}F{F}" for L, F in SMALL])
def test_small_grid_render_and_field_fwd_vs_oracle(ops, LF, H, use_sdf, half):
    L, F = LF
    p = shape_params(L, F, H, use_sdf, half)
    fs = to_spec(ops, p, half)
    for R, S in ((37, 40), (9, 7), (5, 1)):  # ragged last tile, S < 16, one sample per ray
        o, d, area, s, e = sample_rays(R, S, seed=R + S)[:5]
        ref = O.render_rays(p, o, d, area, s, e)
        feats, depth, acc, w = ops.render_fwd(fs, dev(o), dev(d), dev(area), dev(s), dev(e), return_weights=True)
        assert rel_l2(host(feats), ref["features"]) < TIGHT, (R, S)
        assert rel_l2(host(acc), ref["accumulation"]) < TIGHT, (R, S)
        assert rel_l2(host(w), ref["weights"]) < TOL, (R, S)
        assert rel_l2(host(depth), ref["depth"]) < TOL or np.abs(host(depth) - ref["depth"]).max() < 1e-5
        f2, sdf2, head2 = ops.field_fwd(fs, dev(o), dev(d), dev(area), dev(s), dev(e))
        assert rel_l2(host(f2), ref["feature"]) < TIGHT, (R, S)
        assert rel_l2(host(sdf2), ref["sdf"] if use_sdf else np.log(ref["density"])) < TOL
        assert rel_l2(host(head2), ref["alpha"] if use_sdf else ref["density"]) < TOL
        # a processing order changes nothing
        order = ops.ray_order(dev(o), dev(d), 100.0)
        fo, do_, ao = ops.render_fwd(fs, dev(o), dev(d), dev(area), dev(s), dev(e), order=order)
        for a, b in ((fo, feats), (do_, depth), (ao, acc)):
            assert torch.equal(a, b)
        # early ray termination stays within its bound: what a ray skips weighs less than eps in total
        eps = 1e-2
        fe, de, ae = ops.render_fwd(fs, dev(o), dev(d), dev(area), dev(s), dev(e), early_stop_eps=eps)
        assert float((ae - acc).abs().max()) <= eps + 1e-6, (R, S)
        assert float((fe - feats).abs().max()) <= eps * float(np.abs(ref["feature"]).max()) + 1e-5, (R, S)


def test_small_grid_training_forward_saves_the_dense_encoding(ops):
    """save_enc is [N, L*F] in the dense order (the ABI), whatever the kernel's frame"""
    for L, F in SMALL:
        p = shape_params(L, F, 32, True)
        fs = to_spec(ops, p)
        o, d, area, s, e = sample_rays(11, 21, seed=3)[:5]
        (feat, sdf, head), (enc, hg, xf, hf) = ops.field_fwd_train(fs, dev(o), dev(d), dev(area), dev(s), dev(e))
        assert enc.shape == (11 * 21, L * F)
        ref = O.encode_static(p.grid, 100.0, o, d, area, s, e)
        assert rel_l2(host(enc), ref) < TIGHT, (L, F)
        assert rel_l2(host(feat), O.field_fwd(p, o, d, area, s, e)["feature"].reshape(-1, 32)) < TIGHT, (L, F)


# ---- 2. + 3. the field module on the reference's fixtures -------------------------------------------------------------
def make_field(tag, half=False, actors=None):
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    L, F, mn, mx, lg, _ = SHAPES[tag]
    cfg = NeuRADFieldConfig()
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, mn, mx, lg
    cfg.grid.actor.hashgrid_dim, cfg.grid.actor.num_levels, cfg.grid.actor.log2_hashmap_size = 2, 2, 9
    return load_field_weights(NeuRADField(cfg, actors=actors, static_scale=100.0).cuda(), tagged_field_params(tag), half)


def samples(g):
    from neurad_studio_amd.model_components.ray_samplers import PowerSampler

    rs = PowerSampler(num_samples=g["starts"].shape[1], lambda_=-1.0, scaling=0.1).eval()(bundle(g["o"], g["d"], g["area"]))
    assert rel_l2(host(rs.frustums.starts[..., 0]), g["starts"]) < 1e-5
    return rs


def field_grads(fld):
    return {n: p.grad.detach().clone() for n, p in fld.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("tag", ["tiny", "neurad_tiny"])
def test_small_grid_field_vs_reference_golden(tag):
    """Field.forward (no-grad kernel and FieldTrainFn) and render() on the reference's outputs; FieldTrainFn's table, MLP
    and beta gradients against the reference's autograd"""
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH

    g = load_golden(f"field_{tag}")
    fld = make_field(tag).eval()
    assert fld.fused_supported() and fld.fused_supported(with_actors=True)
    rs = samples(g)
    with torch.no_grad():
        out_e = fld(rs)
    out = fld(rs)  # FieldTrainFn
    for o_ in (out_e, out):
        assert rel_l2(host(o_[FH.FEATURE]), g["feature"]) < TOL
        assert rel_l2(host(o_[FH.SDF][..., 0]), g["sdf"]) < TOL
        assert rel_l2(host(o_[FH.ALPHA][..., 0]), g["alpha"]) < TOL
    ((out[FH.FEATURE] * dev(g["g_feature"])).sum() + (out[FH.ALPHA][..., 0] * dev(g["g_head"])).sum()).backward()
    L, F, _, _, lg, _ = SHAPES[tag]
    tg = np.zeros((L * 2**lg, F), np.float32)
    tg[g["tg_idx"]] = g["tg_val"]
    assert rel_l2(host(fld.hashgrid.static_grid.hash_table.grad), tg) < TOL
    for k, l in enumerate(fld.mlp_geo.layers):
        assert rel_l2(host(l.weight.grad), g[f"geo_dw{k}"]) < TOL and rel_l2(host(l.bias.grad), g[f"geo_db{k}"]) < TOL
    for k, l in enumerate(fld.mlp_feature.layers):
        assert rel_l2(host(l.weight.grad), g[f"feat_dw{k}"]) < TOL and rel_l2(host(l.bias.grad), g[f"feat_db{k}"]) < TOL
    assert rel_l2(host(fld.sdf_to_density.beta.grad), g["dbeta"]) < TOL
    # composited: render() against the reference's per-sample outputs, composited by the oracle
    w, _ = O.render_weight_from_alpha(g["alpha"])
    want = O.composite(w, g["feature"], g["starts"], g["ends"])
    with torch.no_grad():
        feats, depth, acc = fld.render(dev(g["o"]), dev(g["d"]), dev(g["area"]), dev(g["starts"]), dev(g["ends"]))
    for got, exp in zip((feats, depth, acc), want):
        assert rel_l2(host(got), exp) < TOL


@pytest.mark.parametrize("tag", ["tiny", "neurad_tiny"])
def test_small_grid_fused_training_vs_operator_path(tag):
    """FieldTrainFn against the operator-level path of the same field (fused_training = False): outputs and every
    parameter gradient, and the ray gradients when the rays require grad"""
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH
    from neurad_studio_amd.model_components.ray_samplers import PowerSampler

    g = load_golden(f"field_{tag}")
    res = {}
    for mode in ("fused", "operator"):
        fld = make_field(tag).eval()
        fld.fused_training = mode == "fused"
        rb = bundle(g["o"], g["d"], g["area"])
        rb.origins.requires_grad_(True), rb.directions.requires_grad_(True)
        rs = PowerSampler(num_samples=g["starts"].shape[1], lambda_=-1.0, scaling=0.1).eval()(rb)
        out = fld(rs)
        ((out[FH.FEATURE] * dev(g["g_feature"])).sum() + (out[FH.ALPHA][..., 0] * dev(g["g_head"])).sum()).backward()
        res[mode] = (host(out[FH.FEATURE]), host(out[FH.ALPHA]), field_grads(fld), host(rb.origins.grad),
                     host(rb.directions.grad))
    (ff, fa, fg, fo, fd), (of, oa, og, oo, od) = res["fused"], res["operator"]
    assert rel_l2(ff, of) < 1e-5 and rel_l2(fa, oa) < 1e-5
    assert set(fg) == set(og)
    for n in fg:
        assert rel_l2(host(fg[n]), host(og[n])) < 5e-5, n
    # (ray gradients sum heavily cancelling per-sample terms: test_gpu_ray_grads.py bounds them against the reference)
    assert rel_l2(fo, oo) < 1e-2 and rel_l2(fd, od) < 1e-2, (rel_l2(fo, oo), rel_l2(fd, od))


@pytest.mark.parametrize("tag", ["tiny", "neurad_tiny"])
def test_small_grid_render_train_vs_operator_path(tag):
    """render_train (the model's fused node: field -> learnable-beta SDF head -> weights -> compositing) against the
    operator-level field (fused_training = False) composited by torch ops in fp64: outputs and every parameter gradient"""
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH

    g = load_golden(f"field_{tag}")
    rs = samples(g)
    edges = torch.cat([rs.frustums.starts[..., 0], rs.frustums.ends[:, -1:, 0]], -1).contiguous()
    R, S = g["starts"].shape
    gF, gD = dev(synth.normal((R, 32), 81)), dev(synth.normal((R, 1), 82))
    gA, gW = dev(synth.normal((R, 1), 83)), dev(synth.normal((R, S - 1), 84))
    res = {}
    for mode in ("fused", "operator"):
        fld = make_field(tag)
        if mode == "fused":
            feats, depth, acc, w = fld.render_train(dev(g["o"]), dev(g["d"]), dev(g["area"]), edges)
        else:
            fld.fused_training = False
            out = fld(rs)
            sd = fld.sdf_to_density
            _, w, feats, depth, acc = torch_sdf_render(out[FH.SDF][..., 0].double(), sd.beta.double(), sd.beta_min_value,
                                                       out[FH.FEATURE].double(), edges.double())
        ((feats * gF).sum() + (depth * gD).sum() + (acc * gA).sum() + (w * gW).sum()).backward()
        res[mode] = ([host(t).astype(np.float64) for t in (feats, depth, acc, w)], field_grads(fld))
    for a, b in zip(res["fused"][0], res["operator"][0]):
        assert rel_l2(a, b) < 2e-5
    # ... and the composited outputs are the reference's (its per-sample outputs composited by the oracle)
    wr, _ = O.render_weight_from_alpha(g["alpha"])
    for got, exp in zip(res["fused"][0][:3], O.composite(wr, g["feature"], g["starts"], g["ends"])):
        assert rel_l2(got, exp) < TOL
    gf, go = res["fused"][1], res["operator"][1]
    assert set(gf) == set(go) and "sdf_to_density.beta" in gf, set(gf) ^ set(go)
    for n in gf:  # (beta's gradient sums every sample's heavily cancelling terms)
        bound = 1e-3 if n == "sdf_to_density.beta" else 2e-4
        assert rel_l2(host(gf[n]), host(go[n])) < bound, (n, rel_l2(host(gf[n]), host(go[n])))


@pytest.mark.parametrize("tag", ["tiny", "neurad_tiny"])
def test_small_grid_fp16_tables_equal_rounded_fp32_tables(tag):
    g = load_golden(f"field_{tag}")
    outs = []
    for half in (False, True):
        fld = make_field(tag).eval()
        rounded = fld.hashgrid.static_grid.hash_table.data.half()
        fld.hashgrid.static_grid.hash_table.data = rounded if half else rounded.float()
        with torch.no_grad():
            outs.append(fld.render(dev(g["o"]), dev(g["d"]), dev(g["area"]), dev(g["starts"]), dev(g["ends"]),
                                   return_weights=True))
            outs[-1] = (*outs[-1], *fld(samples(g)).values())
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 4. NeuRAD tiny with dynamic actors --------------------------------------------------------------------------------
def make_actor_field():
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    fld = make_field("neurad_tiny", actors=actors)
    with torch.no_grad():
        for i, gr in enumerate(fld.hashgrid.actor_grids):
            gr.hash_table.copy_(dev(synth.hash_table(2 * 2**9, 2, seed=400 + i, scale=0.7)))
    return fld


def test_neurad_tiny_render_with_actors_vs_reference_golden():
    g = load_golden("field_neurad_tiny_actors")
    fld = make_actor_field().eval()
    assert fld.fused_supported(with_actors=True)
    with torch.no_grad():
        feats, depth, acc, w = fld.render(dev(g["o"]), dev(g["d"]), dev(g["area"]), dev(g["starts"]), dev(g["ends"]),
                                          return_weights=True, times=dev(g["times"]))
    wr, _ = O.render_weight_from_alpha(g["alpha"])
    want_f, want_d, want_a = O.composite(wr, g["feature"], g["starts"], g["ends"])
    assert rel_l2(host(feats), want_f) < TOL
    assert rel_l2(host(acc), want_a) < TOL
    assert rel_l2(host(depth), want_d) < TOL
    assert rel_l2(host(w), wr) < TOL
    # the oracle agrees (pinned by test_oracle_field_shapes), and the scene has rays with and without candidates
    ref = O.field_fwd_actors(tagged_field_params("neurad_tiny"), actor_params(g, 2, 2), g["o"], g["d"], g["area"], g["starts"],
                             g["ends"], g["times"])
    assert rel_l2(ref["feature"], g["feature"]) < 1e-5
    cnt = fld.hashgrid.prepare_actors(dev(g["o"]), dev(g["d"]), dev(g["area"]), dev(g["starts"]), dev(g["ends"]),
                                      dev(g["times"]))[1][0]
    assert 0 < int((cnt > 0).sum()) < cnt.numel() and len(g["hit_ray"]) > 0


def tiny_model(actors=False, appearance_dim=0):
    """NeuRADHotPath with the "NeuRAD tiny" field: static grid 4 x 2, actor grids 2 x 2 (small tables)"""
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
    from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig

    torch.manual_seed(1)
    c = NeuRADHotPathConfig(appearance_dim=appearance_dim)
    st, ac = c.field.grid.static, c.field.grid.actor
    st.hashgrid_dim, st.num_levels, st.log2_hashmap_size = 2, 4, 12
    ac.hashgrid_dim, ac.num_levels, ac.log2_hashmap_size = 2, 2, 10
    c.field.sdf_beta = 3.0
    for pf in (c.sampling.proposal_field_1, c.sampling.proposal_field_2):
        pf.grid.static.log2_hashmap_size = 11
        pf.grid.actor.log2_hashmap_size = 9
    act = DynamicActors(DynamicActorsConfig(), trajectories=trajectories()) if actors else None
    m = NeuRADHotPath(c, static_scale=100.0, num_sensors=2, duration=4.0, actors=act).cuda()
    with torch.no_grad():
        m.field.hashgrid.static_grid.hash_table.mul_(500.0)
        for gr in m.field.hashgrid.actor_grids:
            gr.hash_table.mul_(3000.0)
        for p in m.proposal_fields:
            p.hashgrid.static_grid.hash_table.mul_(500.0)
            for gr in p.hashgrid.actor_grids:
                gr.hash_table.mul_(2000.0)
    return m


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_neurad_tiny_model_with_actors_training_matches_operator_path():
    """the model's fused training node with dynamic actors (nrhip_field_fwd_train_ovr, override rows [P, 8]) against the
    operator-level path of the same model: outputs and every gradient (static and actor tables, trajectories, MLPs, beta)"""

    res = {}
    for mode in ("fused", "operator"):
        m = tiny_model(actors=True, appearance_dim=16).train()
        m.sampler.eval()
        m.fused_training = mode == "fused"
        assert m.fused_training_possible() == (mode == "fused")
        torch.manual_seed(77)
        out = m.get_nff_outputs(actor_rays())
        (out["features"].square().mean() + 1e-3 * out["depth"].mean() + out["accumulation"].mean()).backward()
        res[mode] = (out, _grads(m))
    for k in ("features", "depth", "accumulation"):
        assert rel_l2(host(res["fused"][0][k]), host(res["operator"][0][k])) < 5e-5, k
    gf, go = res["fused"][1], res["operator"][1]
    assert set(gf) == set(go), set(gf) ^ set(go)
    assert any("field.hashgrid.actor_grids." in n and float(gf[n].abs().sum()) > 0 for n in gf)
    for n in gf:
        assert rel_l2(host(gf[n]), host(go[n])) < 2e-4, (n, rel_l2(host(gf[n]), host(go[n])))


@pytest.mark.parametrize("LF", [(4, 4), (4, 8)], ids=["L4F4", "L4F8"])
def test_four_level_grids_without_actor_kernels_render_through_the_operator_path(LF):
    """4 x 4 (num_levels = 4 at the default hashgrid_dim) and 4 x 8 with dynamic actors: the fused kernels with actors
    exist for 4 x 2 only, so the field keeps the operator-level path -- same numbers as the oracle, no error"""
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
    from neurad_studio_amd.model_components.ray_samplers import PowerSampler

    L, F = LF
    cfg = NeuRADFieldConfig()
    cfg.grid.static.num_levels, cfg.grid.static.hashgrid_dim, cfg.grid.static.log2_hashmap_size = L, F, 10
    cfg.grid.actor.num_levels, cfg.grid.actor.hashgrid_dim, cfg.grid.actor.log2_hashmap_size = 4, F, 9
    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    fld = NeuRADField(cfg, actors=actors, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.mul_(1000.0)
        for gr in fld.hashgrid.actor_grids:
            gr.hash_table.mul_(3000.0)
    assert not fld.fused_supported(with_actors=True)
    rb = actor_rays(64)
    rb.nears, rb.fars = torch.zeros(64, 1, device="cuda"), torch.full((64, 1), 60.0, device="cuda")
    rs = PowerSampler(num_samples=24, lambda_=-1.0, scaling=0.1).eval()(rb)
    with torch.no_grad():
        out = fld(rs)
    o, d, area, t = host(rb.origins), host(rb.directions), host(rb.pixel_area[:, 0]), host(rb.times[:, 0])
    st, en = host(rs.frustums.starts[..., 0]), host(rs.frustums.ends[..., 0])
    ap = O.ActorParams(host(actors.unique_timestamps), host(actors.actor_positions), host(actors.actor_rotations_6d),
                       host(actors.actor_present_at_time), host(actors.actor_sizes), host(actors.actor_padding),
                       [O.GridParams(host(gr.hash_table), 4, 64, 1024, 9) for gr in fld.hashgrid.actor_grids],
                       actor_scale=10.0)
    p = O.FieldParams(O.GridParams(host(fld.hashgrid.static_grid.hash_table), L, 32, 8192, 10), 100.0,
                      [host(l.weight) for l in fld.mlp_geo.layers], [host(l.bias) for l in fld.mlp_geo.layers],
                      [host(l.weight) for l in fld.mlp_feature.layers], [host(l.bias) for l in fld.mlp_feature.layers])
    ref = O.field_fwd_actors(p, ap, o, d, area, st, en, t)
    mean, _ = O.fast_isotropic_gaussian(o, d, area, st, en)
    b2w, valid = O.actor_boxes2world(ap, t)
    r, _, _ = O.actor_hits(ap, mean, b2w, valid, O.pose_inverse(b2w))
    assert len(r) > 0  # samples inside the boxes: the actor branch runs
    assert rel_l2(host(out[FH.FEATURE]), ref["feature"]) < TOL
    assert rel_l2(host(out[FH.ALPHA][..., 0]), ref["alpha"]) < TOL
    with pytest.raises(NotImplementedError):
        fld.render(rb.origins, rb.directions, rb.pixel_area[:, 0], rs.frustums.starts[..., 0].contiguous(),
                   rs.frustums.ends[..., 0].contiguous(), times=rb.times[:, 0])


# ---- 5. model level ----------------------------------------------------------------------------------------------------
def test_neurad_tiny_model_fused_eval_and_training_match_operator_path():
    m = tiny_model().eval()
    R = 64
    o, d, area, _ = synth.rays(R, 9)
    with torch.no_grad():
        assert m.fused_eval_possible()
        out = m.get_outputs_for_ray_bundle(bundle(o, d, area / 9))
        m.fused_eval = False
        assert not m.fused_eval_possible()
        ref = m.get_outputs_for_ray_bundle(bundle(o, d, area / 9))
    for k in ("features", "depth", "accumulation"):
        assert rel_l2(host(out[k]), host(ref[k])) < 2e-5, k
    res = {}
    for mode in ("fused", "operator"):
        m = tiny_model().train()
        m.sampler.eval()
        m.fused_training = mode == "fused"
        assert m.fused_training_possible() == (mode == "fused")
        out = m.get_nff_outputs(bundle(o, d, area / 9))
        (out["features"].square().mean() + 1e-3 * out["depth"].mean() + out["accumulation"].mean()).backward()
        res[mode] = (out, _grads(m))
    for k in ("features", "depth", "accumulation"):
        assert rel_l2(host(res["fused"][0][k]), host(res["operator"][0][k])) < 2e-5, k
    gf, go = res["fused"][1], res["operator"][1]
    assert set(gf) == set(go)
    for n in gf:  # (beta's gradient is a heavily cancelling sum: the bound of the actor-scene test)
        assert rel_l2(host(gf[n]), host(go[n])) < 2e-4, (n, rel_l2(host(gf[n]), host(go[n])))


# ---- 6. shapes outside the set -----------------------------------------------------------------------------------------
def test_uninstantiated_shapes_stay_unsupported_and_the_field_falls_back(ops):
    from neurad_studio_amd import _lib
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    for L, F, H in ((3, 8, 32), (4, 2, 48), (2, 2, 32)):
        p = shape_params(4, 2, H, True) if (L, F) == (4, 2) else None
        if p is None:
            p = field_params(True, L, F, 10, H, 32, 2048, scale=1e-3, seed=5)
        fs = to_spec(ops, p)
        o, d, area, s, e = sample_rays(4, 8, seed=1)[:5]
        # NRHIP_ERR_UNSUPPORTED (2) from the C entry points, with a message that names the shape
        with pytest.raises(_lib.NeuradHipError, match=rf"code 2\).*L={L} F={F} H={H}"):
            ops.render_fwd(fs, dev(o), dev(d), dev(area), dev(s), dev(e))
        with pytest.raises(_lib.NeuradHipError, match=rf"code 2\).*L={L} F={F} H={H}"):
            ops.field_fwd_train(fs, dev(o), dev(d), dev(area), dev(s), dev(e))
    # the field with such a grid runs the operator-level path, no error
    cfg = NeuRADFieldConfig()
    cfg.grid.static.num_levels, cfg.grid.static.hashgrid_dim, cfg.grid.static.log2_hashmap_size = 3, 8, 10
    fld = NeuRADField(cfg, actors=None, static_scale=100.0).cuda().eval()
    assert not fld.fused_supported() and not fld.fused_supported(with_actors=True)
    o, d, area, _ = synth.rays(6, 2)
    from neurad_studio_amd.model_components.ray_samplers import PowerSampler

    rs = PowerSampler(num_samples=9, lambda_=-1.0, scaling=0.1).eval()(bundle(o, d, area))
    with torch.no_grad():
        out = fld(rs)
    assert out[FH.FEATURE].shape == (6, 9, 32) and torch.isfinite(out[FH.FEATURE]).all()
    with pytest.raises(NotImplementedError):
        fld.render(dev(o), dev(d), dev(area), rs.frustums.starts[..., 0].contiguous(), rs.frustums.ends[..., 0].contiguous())
