"""Model-level glue of the hot path on the GPU against outputs of the reference's own NeuRADModel
(tests/golden/model_train_glue.npz, tests/golden/proposal_actors.npz -- oracle/make_golden_model.py):
appearance embedding (C3), is_close_to_lidar / proposal carving terms / non_nearby outputs (C4), the lidar head, the
lidar loss terms and the proposal field's actor gradients."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
from builders import trajectories
from gpu_util import cuda, glue_bundle, glue_model, host

pytestmark = pytest.mark.gpu
TOL = 1e-4


def test_training_outputs_with_lidar_metadata_and_appearance_vs_reference():
    """the OPERATOR-level training path (the reference's orchestration over this package's fields / sampler / renderers);
    the fused training nodes are held against the same golden in tests/test_gpu_train_fused.py"""
    g = load_golden("model_train_glue")
    m = glue_model(g).train()
    m.fused_training = False
    m.sampler.eval(), m.field.eval()  # deterministic sampling, as in the generator
    for p in m.proposal_fields:
        p.eval()
    out = m.get_nff_outputs(glue_bundle(g), calc_lidar_losses=True)
    assert out["features"].shape == (80, 48)
    for k in ("features", "depth", "accumulation", "prop_depth_0", "prop_depth_1"):
        assert rel_l2(host(out[k]), g[k]) < TOL, k
    for i in range(3):
        assert rel_l2(host(out["weights_list"][i][..., 0]), g[f"weights_{i}"]) < TOL
        close = host(out["ray_samples_list"][i].metadata["is_close_to_lidar"][..., 0])
        # a sample within float rounding of the 0.1 m carving band may flip: allow a handful
        assert (close != g[f"close_{i}"]).sum() <= 2, i
    for i in range(2):
        assert abs(float(out[f"prop_weights_loss_{i}"]) / float(g[f"prop_weights_loss_{i}"]) - 1) < 1e-3
    assert abs(out["non_nearby_weights"].shape[0] - g["non_nearby_weights"].shape[0]) <= 2
    if out["non_nearby_weights"].shape == g["non_nearby_weights"].shape:
        assert rel_l2(host(out["non_nearby_weights"]), g["non_nearby_weights"]) < TOL
        np.testing.assert_array_equal(host(out["non_nearby_lidar_ray_indices"]), g["non_nearby_lidar_ray_indices"])
    # ---- lidar head + lidar losses ----
    from neurad_studio_amd.model_components.lidar_losses import LidarLossSettings, lidar_loss_dict, lidar_metrics
    from neurad_studio_amd.model_components.losses import distortion_loss, zipnerf_interlevel_loss

    is_lidar = cuda(g["is_lidar"])
    intensity, logits = m.decode_lidar(out["features"], is_lidar)
    assert rel_l2(host(intensity), g["intensity"]) < TOL and rel_l2(host(logits), g["ray_drop_logits"]) < TOL
    outputs = dict(out, intensity=intensity, ray_drop_logits=logits)
    cfg = LidarLossSettings()
    lc = g["loss_cfg"]
    assert (cfg.depth_mult, cfg.intensity_mult, cfg.carving_mult, cfg.ray_drop_loss_mult, cfg.prop_lidar_loss_mult,
            cfg.non_return_loss_mult, cfg.non_return_lidar_distance, cfg.quantile_threshold) == tuple(lc[:8])
    did_return = cuda(g["did_return"])[is_lidar]
    metrics = lidar_metrics(outputs, is_lidar, did_return, cuda(g["directions_norm"])[is_lidar][:, None],
                            cuda(g["lidar_points"])[:, 3:4], cfg, fused=False)
    for k in ("depth_loss", "intensity_loss", "ray_drop_loss", "carving_loss", "depth_loss_0", "depth_loss_1",
              "carving_loss_0", "carving_loss_1"):
        assert abs(float(metrics[k]) / float(g["metric_" + k]) - 1) < 2e-3, (k, float(metrics[k]), float(g["metric_" + k]))
    losses = lidar_loss_dict(metrics, cfg)
    for k, v in losses.items():
        assert abs(float(v) / float(g["loss_" + k]) - 1) < 2e-3, k
    losses["interlevel_loss"] = float(lc[9]) * zipnerf_interlevel_loss(out["weights_list"], out["ray_samples_list"])
    losses["distortion_loss"] = float(lc[10]) * distortion_loss(out["weights_list"], out["ray_samples_list"])
    assert abs(float(losses["interlevel_loss"]) / float(g["loss_interlevel_loss"]) - 1) < 2e-3
    assert abs(float(losses["distortion_loss"]) / float(g["loss_distortion_loss"]) - 1) < 2e-3
    # the whole chain backward: the gradients the reference's autograd produced for the same total loss.  The bounds below
    # (2e-3, 5e-3 for beta) are set by the REFERENCE's own fp32 noise on a batch of this size, not by these kernels: its
    # model in fp32 differs from itself in fp64 by up to 5e-3 on the table / MLP gradients of the lidar terms -- a handful
    # of hidden units within 5e-5 of the ReLU kink flip, each switching one sample's whole contribution -- while its loss
    # values agree to 1e-7 (oracle/grad_noise_floor.py, profiles/r04_grad_noise_floor.json).  The tight statement about the
    # same kernels is tests/test_gpu_reference_plugin.py: per loss term, rgb / interlevel gradients within 2e-4.
    sum(losses.values()).backward()
    assert rel_l2(host(m.lidar_decoder.layers[0].weight.grad), g["g_lidar_decoder_w0"]) < 2e-3
    assert rel_l2(host(m.appearance_embedding.weight.grad), g["g_embedding"]) < 2e-3
    assert abs(float(m.field.sdf_to_density.beta.grad) / float(g["g_beta"]) - 1) < 5e-3
    # the two table gradients of the composed step, element by element (the golden stores them sparse)
    for t, key in ((m.field.hashgrid.static_grid.hash_table, "g_field_table"),
                   (m.proposal_fields[1].hashgrid.static_grid.hash_table, "g_prop1_table")):
        dense = np.zeros(t.numel(), np.float32)
        dense[g[key + "_idx"]] = g[key + "_val"]
        assert rel_l2(host(t.grad).reshape(-1), dense) < 2e-3, key
    assert m.proposal_fields[0].hashgrid.static_grid.hash_table.grad is None  # the late-binding quirk


def test_eval_fused_path_with_appearance_and_normalized_depth():
    """C3 through the fused eval path, and normalize_depth (DepthRenderer('expected'), renderers.py:398-416) against
    the operator-level path of the same model."""
    g = load_golden("model_train_glue")
    m = glue_model(g).eval()
    with torch.no_grad():
        fused = m.get_nff_outputs(glue_bundle(g))
    op = m.get_nff_outputs(glue_bundle(g))  # grad enabled -> operator-level path, eval mode (no jitter)
    assert fused["features"].shape == (80, 48)
    for k in ("features", "depth", "accumulation", "prop_depth_0", "prop_depth_1"):
        assert rel_l2(host(fused[k]), host(op[k])) < 5e-5, k
    assert rel_l2(host(fused["features"][:, 32:]), g["features"][:, 32:]) < 1e-5  # the embedding part is mode independent
    from neurad_studio_amd.model_components.renderers import DepthRenderer

    m.config.normalize_depth, m.renderer_depth = True, DepthRenderer(method="expected")
    with torch.no_grad():
        fused_n = m.get_nff_outputs(glue_bundle(g))
    op_n = m.get_nff_outputs(glue_bundle(g))
    assert rel_l2(host(fused_n["depth"]), host(op_n["depth"])) < 5e-5
    assert bool((fused_n["depth"] >= fused["depth"] - 1e-6).all())  # dividing by sum w <= 1 never shortens a depth
    # early termination and ray ordering are eval options of the same path: bounded / no change
    from neurad_studio_amd.model_components.renderers import render_depth_simple

    del m.renderer_depth  # (an nn.Module attribute cannot be overwritten by a plain function)
    m.config.normalize_depth, m.renderer_depth = False, render_depth_simple
    m.order_rays = True
    with torch.no_grad():
        ordered = m.get_nff_outputs(glue_bundle(g))
    assert torch.equal(ordered["features"], fused["features"]) and torch.equal(ordered["depth"], fused["depth"])
    m.early_stop_eps = 1e-3
    with torch.no_grad():
        cut = m.get_nff_outputs(glue_bundle(g))
    assert float((cut["accumulation"] - fused["accumulation"]).abs().max()) <= 1.01e-3


def test_proposal_field_with_actors_density_and_gradients_vs_reference():
    """require_actor_grad=False keeps the POSES out of the graph only -- the proposal fields' actor
    grids and decoder train through the in-box samples.  Golden = the reference's autograd."""
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.fields.neurad_field import NeuRADProposalField, NeuRADProposalFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
    from neurad_studio_amd.model_components.ray_samplers import PowerSampler
    import synth

    g = load_golden("proposal_actors")
    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    cfg = NeuRADProposalFieldConfig()
    cfg.grid.static.log2_hashmap_size = 10
    cfg.grid.actor.log2_hashmap_size = 8
    fld = NeuRADProposalField(cfg, actors=actors, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.copy_(cuda(synth.hash_table(6 * 2**10, 1, seed=61, scale=2.0)))
        for i, gr in enumerate(fld.hashgrid.actor_grids):
            gr.hash_table.copy_(cuda(synth.hash_table(4 * 2**8, 1, seed=500 + i, scale=2.5)))
        fld.density_decoder.weight.copy_(cuda(synth.uniform((1, 6), -0.6, 0.6, seed=62)))
    R = g["o"].shape[0]
    rb = RayBundle(origins=cuda(g["o"]), directions=cuda(g["d"]), pixel_area=torch.full((R, 1), 2.43e-6, device="cuda"),
                   times=cuda(g["times"])[:, None], nears=torch.zeros(R, 1, device="cuda"),
                   fars=torch.full((R, 1), 60.0, device="cuda"))
    rs = PowerSampler(num_samples=40, lambda_=-1.0, scaling=0.1).eval()(rb)
    with torch.no_grad():
        d0, _ = fld.get_density(rs)
    assert rel_l2(host(d0[..., 0]), g["density"]) < TOL
    dens, _ = fld.get_density(rs)
    assert rel_l2(host(dens[..., 0]), g["density"]) < TOL
    (dens[..., 0] * cuda(g["g_density"])).sum().backward()
    tg = host(fld.hashgrid.static_grid.hash_table.grad)
    ref_tg = np.zeros_like(tg)
    ref_tg[g["tg_idx"]] = g["tg_val"]
    assert rel_l2(tg, ref_tg) < TOL
    assert rel_l2(host(fld.density_decoder.weight.grad), g["g_decoder"]) < TOL
    for i, gr in enumerate(fld.hashgrid.actor_grids):
        ref_g = g[f"ag{i}"]
        got = np.zeros_like(ref_g) if gr.hash_table.grad is None else host(gr.hash_table.grad)
        assert np.abs(ref_g).sum() == 0 or rel_l2(got, ref_g) < TOL, i
    assert any(np.abs(g[f"ag{i}"]).sum() > 0 for i in range(3)), "the golden must exercise the actor grids"
    assert bool(g["dpos_is_none"]) and actors.actor_positions.grad is None  # poses stay out of the graph


def test_rgb_cnn_decoder_vs_reference():
    """the RGB decoder behind the camera rays: same module tree / state_dict names as the reference's
    rgb_decoder, outputs of its training-mode (batch-statistics BN) and eval-mode forward on two 8x8 feature patches --
    through the torch modules (fp32) and through the HIP kernels (fp16 operands)."""
    import synth
    from neurad_studio_amd.model_components.cnns import decode_rgb, make_rgb_decoder

    g = load_golden("cnn_decoder")
    dec = make_rgb_decoder(48, 32, 3).cuda()
    assert [n for n, _ in dec.named_parameters()] == list(g["param_names"])
    with torch.no_grad():
        for k, (name, p) in enumerate(dec.named_parameters()):  # the generator's rule (oracle/make_golden_model.py)
            fan_in = p[0].numel() if p.dim() > 1 else 1
            w = (synth.normal(tuple(p.shape), 600 + k) * (1.0 / np.sqrt(fan_in) if p.dim() > 1 else 0.1)).astype(np.float32)
            if name.endswith(("1.weight", "4.weight")) and p.dim() == 1:
                w = w + 1.0
            p.copy_(cuda(w))
    feats = cuda(g["features"])
    import copy

    # (1) the torch modules in fp32: the golden's own arithmetic
    d32 = copy.deepcopy(dec).train()
    rgb = decode_rgb(d32, feats, (8, 8), fused=False)
    assert rgb.shape == (2, 24, 24, 3) and rel_l2(host(rgb), g["rgb_train"]) < TOL
    assert rel_l2(host(d32[2].main_branch[1].running_mean), g["bn_running_mean"]) < TOL
    d32.eval()
    with torch.no_grad():
        assert rel_l2(host(decode_rgb(d32, feats, (8, 8), fused=False)), g["rgb_eval"]) < TOL
    # (2) the HIP kernels (csrc/decoder.hip): fp16 operands, fp32 accumulation -- the reference trainer's mixed precision,
    # while the golden is the reference's fp32 forward.  Tolerance: torch autocast(fp16) on the same modules is the yardstick
    # (measured 1.0e-3 rel-L2 on this golden); 3e-3 bounds both.
    FP16_TOL = 3e-3
    dec.train()
    rgb = decode_rgb(dec, feats, (8, 8))
    assert rgb.shape == (2, 24, 24, 3) and rgb.dtype == torch.float32 and rel_l2(host(rgb), g["rgb_train"]) < FP16_TOL
    assert rel_l2(host(dec[2].main_branch[1].running_mean), g["bn_running_mean"]) < FP16_TOL
    assert int(dec[2].main_branch[1].num_batches_tracked) == 1
    dec.eval()
    with torch.no_grad():
        assert rel_l2(host(decode_rgb(dec, feats, (8, 8))), g["rgb_eval"]) < FP16_TOL
    d16 = copy.deepcopy(d32).train()
    with torch.autocast("cuda", dtype=torch.float16):
        ra = decode_rgb(d16, feats, (8, 8), fused=False).float()
    print("rel-L2 vs the reference's fp32 forward: HIP", rel_l2(host(rgb), g["rgb_train"]), "autocast", rel_l2(host(ra), g["rgb_train"]))


def test_chunked_eval_entry_and_lidar_head():
    """get_outputs_for_ray_bundle (the chunked entry of models/neurad.py:623-675): chunks of any size give the outputs of
    one call, the lidar head runs on the rendered features; also through the reference's own slicing protocol."""
    g = load_golden("model_train_glue")
    m = glue_model(g).eval()
    with torch.no_grad():
        whole = m.get_nff_outputs(glue_bundle(g))
    out = m.get_outputs_for_ray_bundle(glue_bundle(g), num_rays_per_chunk=32, is_lidar=True)  # 80 rays -> 32 + 32 + 16
    for k in ("features", "depth", "accumulation", "prop_depth_0", "prop_depth_1"):
        assert torch.equal(out[k], whole[k]), k  # per-ray kernels: chunking changes nothing, bit for bit
    intensity, logit = m.decode_lidar(whole["features"])
    assert torch.equal(out["intensity"], intensity) and torch.equal(out["ray_drop_prob"], logit.sigmoid())
    assert out["intensity"].shape == (80, 1) and float(out["intensity"].min()) >= 0 and float(out["intensity"].max()) <= 1

    class RefLikeBundle:  # the reference RayBundle's protocol: __len__ + get_row_major_sliced_ray_bundle (rays.py:293-311)
        def __init__(self, rb):
            self.rb = rb

        def __len__(self):
            return len(self.rb)

        def get_row_major_sliced_ray_bundle(self, a, b):
            from neurad_studio_amd.models.neurad import _slice_bundle
            return _slice_bundle(self.rb, a, b)

    out2 = m.get_outputs_for_ray_bundle(RefLikeBundle(glue_bundle(g)), num_rays_per_chunk=50)
    assert torch.equal(out2["features"], whole["features"]) and "intensity" not in out2


def test_normals_renderer_vs_reference_formula():
    from neurad_studio_amd.model_components.renderers import NormalsRenderer

    torch.manual_seed(3)
    normals = torch.randn(37, 24, 3, device="cuda")
    w = torch.rand(37, 24, 1, device="cuda") * 0.1
    want = torch.sum(w * normals, dim=-2)  # renderers.py:481
    assert rel_l2(host(NormalsRenderer.forward(normals, w, normalize=False)), host(want)) < 1e-6
    want_n = want / (torch.norm(want, dim=-1, keepdim=True) + 1e-10)  # safe_normalize, utils/math.py:468
    assert rel_l2(host(NormalsRenderer()(normals, w)), host(want_n)) < 1e-6


def test_model_eval_with_actors_fused_render_matches_operator_path():
    """A scene with dynamic actors through the model: eval under no_grad takes the fused render kernel with per-sample
    table select (proposal rounds at operator level); the grad-enabled call of the same model takes the operator-level
    path end to end (pinned to the reference by test_gpu_actors / proposal_actors goldens)."""
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
    from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig

    torch.manual_seed(1)
    c = NeuRADHotPathConfig(appearance_dim=0)
    c.field.grid.static.log2_hashmap_size = 12
    c.field.grid.actor.log2_hashmap_size = 10
    c.field.sdf_beta = 3.0
    for pf in (c.sampling.proposal_field_1, c.sampling.proposal_field_2):
        pf.grid.static.log2_hashmap_size = 11
        pf.grid.actor.log2_hashmap_size = 9
    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    m = NeuRADHotPath(c, static_scale=100.0, actors=actors).cuda().eval()
    with torch.no_grad():
        m.field.hashgrid.static_grid.hash_table.mul_(500.0)
        for gr in m.field.hashgrid.actor_grids:
            gr.hash_table.mul_(3000.0)
        for p in m.proposal_fields:
            p.hashgrid.static_grid.hash_table.mul_(500.0)
            for gr in p.hashgrid.actor_grids:
                gr.hash_table.mul_(2000.0)
    R = 256
    gen = torch.Generator().manual_seed(5)
    times = 1.0 + torch.rand(R, 1, generator=gen)  # all three trajectories exist in [1, 2]
    a = torch.arange(R) % 3  # look at actor a, where it is at the ray's time (builders.trajectories), from ~4 m:
    tgt = torch.stack([12.0 + 2.0 * times[:, 0] + a, torch.tensor([8.0, -6.0, -5.0])[a], torch.full((R,), 0.5)], -1)
    side = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen) * torch.tensor([1.0, 1.0, 0.15]), dim=-1)
    o = tgt + 4.0 * side  # the box fills the first metres of the ray, where the samplers put their samples
    d = torch.nn.functional.normalize(tgt + 0.3 * torch.randn(R, 3, generator=gen) - o, dim=-1)
    d[::4] = -d[::4]  # every fourth ray looks away

    def rb():
        return RayBundle(origins=o.cuda(), directions=d.cuda(), pixel_area=torch.full((R, 1), 2.7e-7, device="cuda"),
                         times=times.cuda())

    assert m.fused_eval_possible() is False  # (grad enabled here)
    with torch.no_grad():
        assert m.fused_eval_possible()
        fused = m.get_nff_outputs(rb())
    op = m.get_nff_outputs(rb())
    for k in ("features", "depth", "accumulation", "prop_depth_0", "prop_depth_1"):
        assert rel_l2(host(fused[k]), host(op[k])) < 5e-5, k
    # the proposal rounds see the actors too (fused sampler with per-sample table select): switching the proposal
    # fields' actors off changes the proposal depths; with actors in only ONE of the two fields the model falls back to
    # the operator-level sampler and still agrees with the grad-enabled path
    for p in m.proposal_fields:
        p.hashgrid.config.disable_actors = True
    with torch.no_grad():
        no_prop_actors = m.get_nff_outputs(rb())
    assert rel_l2(host(no_prop_actors["prop_depth_1"]), host(fused["prop_depth_1"])) > 1e-4
    m.proposal_fields[1].hashgrid.config.disable_actors = False
    m.reproduce_late_binding_quirk = False  # round 0 -> field 0 (no actors), round 1 -> field 1 (actors)
    quirk_fns, m.density_fns = m.density_fns, [lambda x, f=f: f.get_density(x)[0] for f in m.proposal_fields]
    with torch.no_grad():
        mixed = m.get_nff_outputs(rb())
    mixed_op = m.get_nff_outputs(rb())
    for k in ("features", "depth", "prop_depth_0", "prop_depth_1"):
        assert rel_l2(host(mixed[k]), host(mixed_op[k])) < 5e-5, k
    m.proposal_fields[0].hashgrid.config.disable_actors = False
    m.reproduce_late_binding_quirk, m.density_fns = True, quirk_fns
    # the actors matter in this scene: without them the rendering differs
    m.field.hashgrid.config.disable_actors = True
    with torch.no_grad():
        static_only = m.get_nff_outputs(rb())
    assert rel_l2(host(static_only["features"]), host(fused["features"])) > 1e-3


def test_config4_shape_actors_fp16_field_tables_appearance_65536_rays_chunked():
    """BASELINE config[4] at full size: NeuRAD-default grids with the main field's tables (static 8 x 2^22 x 4 and 24
    actor grids) in fp16, appearance embedding, dynamic actors, a 65536-ray batch through the chunked eval entry.
    Size-independent properties + a 2048-ray slice against the operator-level path of the same model with fp32 tables
    holding the rounded values (that path is pinned to the reference by test_gpu_actors / the proposal_actors golden)."""
    from neurad_studio_amd import ops
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
    from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig, _slice_bundle

    A, R = 24, 65536
    ts = torch.linspace(0.0, 4.0, 9)
    gen = torch.Generator().manual_seed(21)
    trajs = []
    for a in range(A):
        x0, y0 = 60 * torch.rand(2, generator=gen) - 30
        yaw, v = 6.28 * float(torch.rand(1, generator=gen)), 4 * float(torch.rand(1, generator=gen))
        poses = torch.eye(4).repeat(len(ts), 1, 1)
        c, s = np.cos(yaw), np.sin(yaw)
        poses[:, :3, :3] = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3] = x0 + v * ts * c, y0 + v * ts * s, 0.8
        trajs.append({"timestamps": ts.clone(), "poses": poses, "dims": torch.tensor([2.0, 4.6, 1.6]),
                      "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})

    def build(half):
        torch.manual_seed(2)
        m = NeuRADHotPath(NeuRADHotPathConfig(), static_scale=100.0, num_sensors=6, duration=4.0,
                          actors=DynamicActors(DynamicActorsConfig(), trajectories=trajs)).cuda().eval()
        with torch.no_grad():
            m.field.hashgrid.static_grid.hash_table.mul_(300.0)
            for gr in m.field.hashgrid.actor_grids:
                gr.hash_table.mul_(2000.0)
            for p in m.proposal_fields:
                p.hashgrid.static_grid.hash_table.mul_(500.0)
            for gr in [m.field.hashgrid.static_grid, *m.field.hashgrid.actor_grids]:
                gr.hash_table.data = gr.hash_table.data.half() if half else gr.hash_table.data.half().float()
        return m

    o = torch.randn(R, 3, generator=gen) * torch.tensor([20.0, 20.0, 0.3]) + torch.tensor([0.0, 0.0, 1.5])
    d = torch.randn(R, 3, generator=gen) * torch.tensor([1.0, 1.0, 0.1])
    d = torch.nn.functional.normalize(d, dim=-1)
    rb = RayBundle(origins=o.cuda(), directions=d.cuda(), pixel_area=torch.full((R, 1), 2.7e-7, device="cuda"),
                   times=(4 * torch.rand(R, 1, generator=gen)).cuda(),
                   metadata={"sensor_idxs": torch.randint(0, 6, (R, 1), generator=gen).cuda()})
    m16 = build(True)
    calls = []
    real = ops.render_fwd_actors
    ops.render_fwd_actors = lambda *a, **k: (calls.append(a[3].shape[0]), real(*a, **k))[1]
    try:
        out = m16.get_outputs_for_ray_bundle(rb, num_rays_per_chunk=1 << 15)
        out2 = m16.get_outputs_for_ray_bundle(rb, num_rays_per_chunk=24000)
    finally:
        ops.render_fwd_actors = real
    assert calls[:2] == [1 << 15, 1 << 15] and len(calls) == 2 + 3  # the fused actor kernel rendered every chunk
    assert out["features"].shape == (R, 48) and all(torch.isfinite(v).all() for v in out.values())
    assert float(out["accumulation"].min()) >= -1e-6 and float(out["accumulation"].max()) <= 1 + 1e-5
    for k in out:
        assert torch.equal(out[k], out2[k]), k  # chunking changes nothing
    m32 = build(False)
    sl = _slice_bundle(rb, 1000, 3048)
    op = m32.get_nff_outputs(sl)  # grad enabled -> operator-level path, fp32 tables with the same (rounded) values
    for k in ("features", "depth", "accumulation"):
        assert rel_l2(host(out[k][1000:3048]), host(op[k])) < 5e-5, k
    # ---- and against the ORACLE's actor path (numpy, oracle/neurad_oracle.py: field_fwd_actors -> C1 -> C2) on a 256-ray
    # slice, on the fp16-rounded tables: the fused per-sample table select + MLPs + compositing of this configuration,
    # fed with the samples the fused proposal rounds placed for those rays
    import neurad_oracle as O

    a0, a1 = 2000, 2256
    sl = _slice_bundle(rb, a0, a1)
    with torch.no_grad():
        m16._scale_pixel_area(sl)
        sl.fars = torch.full_like(sl.pixel_area, m16.config.sampling.sky_distance)
        sl.nears = torch.zeros_like(sl.fars)
        so, sd_, st = sl.origins.contiguous(), sl.directions.contiguous(), sl.times.reshape(-1)
        n = sl.nears.reshape(-1)
        _, cand = m16.field.hashgrid.prepare_actors(so, sd_, sl.pixel_area.reshape(-1), torch.stack([n, n + 1], -1),
                                                    torch.stack([n + 1, n + 2], -1), st)
        pf = [m16.proposal_fields[-1]] * 2
        rs, _, _ = m16.sampler.generate_fused(sl, pf, m16.config.sampling.sky_distance, actor_cand=cand)
        starts = rs.frustums.starts[..., 0].contiguous()
        ends = rs.frustums.ends[..., 0].clone()
        ends[:, -1] = m16.config.sampling.sky_distance
        feats, depth, acc = m16.field.render(so, sd_, sl.pixel_area, starts, ends, times=st, actor_cand=cand)[:3]
    f, hg, act = m16.field, m16.field.hashgrid, m16.field.hashgrid.actors
    gcfg = hg.config
    grid = O.GridParams(host(hg.static_grid.hash_table.float()), gcfg.static.num_levels, gcfg.static.base_res,
                        gcfg.static.max_res, gcfg.static.log2_hashmap_size)
    fp = O.FieldParams(grid, 100.0, [host(l.weight) for l in f.mlp_geo.layers], [host(l.bias) for l in f.mlp_geo.layers],
                       [host(l.weight) for l in f.mlp_feature.layers], [host(l.bias) for l in f.mlp_feature.layers],
                       beta=float(f.sdf_to_density.beta), use_sdf=True)
    ap = O.ActorParams(host(act.unique_timestamps), host(act.actor_positions), host(act.actor_rotations_6d),
                       host(act.actor_present_at_time), host(act.actor_sizes), host(act.actor_padding),
                       [O.GridParams(host(hg.actor_grids[i].hash_table.float()), gcfg.actor.num_levels, gcfg.actor.base_res,
                                     gcfg.actor.max_res, gcfg.actor.log2_hashmap_size) for i in act.actor_to_id.tolist()],
                       actor_scale=float(gcfg.actor.actor_scale))
    ref = O.field_fwd_actors(fp, ap, host(so), host(sd_), host(sl.pixel_area.reshape(-1)), host(starts), host(ends), host(st))
    w, _ = O.render_weight_from_alpha(ref["alpha"])
    rf, rd, ra = O.composite(w, ref["feature"], host(starts), host(ends))
    in_box = float((np.abs(ref["directions"] - host(sd_)[:, None, :]).max(-1) > 0).mean())
    assert in_box > 0.005, f"the slice must contain actor samples ({in_box:.4f})"
    assert rel_l2(host(feats), rf) < 1e-4 and rel_l2(host(acc), ra) < 1e-4 and rel_l2(host(depth), rd) < 1e-4
    assert torch.equal(out["features"][a0:a1, :32], feats)  # the chunked entry rendered exactly this
    # ---- round 5: the proposal fields' STATIC tables in fp16 storage too (bench.py --config c4; actor grids stay fp32).  The
    # fused sampler with the per-sample actor select takes them, and places the samples of the same model whose fp32 proposal
    # tables hold the rounded values
    for mm, half in ((m16, True), (m32, False)):
        for pfield in mm.proposal_fields:
            t = pfield.hashgrid.static_grid.hash_table
            t.data = t.data.half() if half else t.data.half().float()
    assert all(pfield.fused_sampler_supported() for pfield in m16.proposal_fields)
    with torch.no_grad():
        got = m16.sampler.generate_fused(sl, [m16.proposal_fields[-1]] * 2, m16.config.sampling.sky_distance, actor_cand=cand)
        want = m32.sampler.generate_fused(sl, [m32.proposal_fields[-1]] * 2, m32.config.sampling.sky_distance, actor_cand=cand)
    for k in range(2):
        assert rel_l2(host(got[1][k]), host(want[1][k])) < 1e-5, k
    assert rel_l2(host(got[0].frustums.starts), host(want[0].frustums.starts)) < 1e-5
