"""The plugin against the reference, as a harness: the ``neurad-hip`` model on the GPU and the reference's torch model on the
CPU with the same weights (build_pair), their batches, one backward per loss term and the reference's own noise floors
(per_loss_gradient_errors, check_gradients_against_floor), the reference's training loop around either model (Loop,
Pipeline) and a synthetic drive for the method's own pipeline (method_config).  Used by tests/test_gpu_reference_plugin.py,
test_gpu_plugin_train_loop.py, test_gpu_plugin_pipeline.py, test_gpu_plugin_trainer.py, test_gpu_replicas.py,
test_reference_integration.py, oracle/grad_noise_floor.py, scripts/plugin_grad_diag.py and scripts/amp_drift_probe.py.

The only substitutions on the reference side are the ones every golden generator makes (oracle/make_golden_model.py): dense
nerfacc 0.5.2 formulas in place of the CPU placeholder (models/neurad.py:713-715 returns 0.5 on CPU), no VGG network
(torchvision weights absent, ``vgg_mult = 0``), samplers and fields in eval mode inside the training-mode model."""
import os
import sys
import types
from collections import defaultdict
from copy import deepcopy
from dataclasses import dataclass, field
from pathlib import Path
from typing import Type

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402
import synth  # noqa: E402
from builders import trajectories  # noqa: E402
from conftest import rel_l2  # noqa: E402,F401  (the scripts read it from here)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))


def N(t):
    return t.detach().float().cpu().numpy()


def N_native(t):
    """(no cast: the tensor's own dtype)"""
    return t.detach().cpu().numpy()


def dense_nerfacc():
    m = types.ModuleType("nerfacc")

    def render_weight_from_alpha(alphas, **kw):
        trans = torch.cumprod(torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas[..., :-1]], -1), -1)
        return trans * alphas, trans

    def accumulate_along_rays(weights, values=None, ray_indices=None, n_rays=None):
        return weights.sum(-1, keepdim=True) if values is None else (weights[..., None] * values).sum(-2)

    def render_weight_from_density(t_starts, t_ends, sigmas, **kw):
        sd = sigmas * (t_ends - t_starts)
        trans = torch.exp(-(torch.cumsum(sd, -1) - sd))
        alphas = 1 - torch.exp(-sd)
        return trans * alphas, trans, alphas

    m.render_weight_from_alpha, m.accumulate_along_rays = render_weight_from_alpha, accumulate_along_rays
    m.render_weight_from_density = render_weight_from_density
    return m


def many_trajectories(n):
    """n actors in two lanes along +x, staggered every 3 m, each present over its own part of the scene's 4 s (config[4]'s 32
    actors at test size: several boxes along every ray, neighbours overlapping at the lane changes)"""
    ts_all = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])
    out = []
    for a in range(n):
        ts = ts_all[a % 2:] if a % 3 else ts_all[:4]
        yaw = 0.25 * ((a * 7) % 5 - 2) / 2
        poses = []
        for t in ts:
            c, s = np.cos(yaw + 0.04 * float(t)), np.sin(yaw + 0.04 * float(t))
            p = torch.eye(4)
            p[:3, :3] = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
            p[:3, 3] = torch.tensor([8.0 + 3.0 * a + 1.5 * float(t), 6.5 if a % 2 == 0 else -5.5, 0.5])
            poses.append(p)
        out.append({"timestamps": ts.clone(), "poses": torch.stack(poses),
                    "dims": torch.tensor([1.9 + 0.01 * a, 4.2 + 0.02 * a, 1.5 + 0.01 * a]),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out


def fill(model):
    """deterministic O(1)-feature parameters (tests/synth.py) so that densities, weights and every loss term are far from
    their trivial values"""
    for k, (name, p) in enumerate(model.named_parameters()):
        if name.endswith("hash_table"):
            scale = 1.0 if p.shape[1] == 4 else 2.5
            p.data = T(synth.hash_table(p.shape[0], p.shape[1], seed=100 + k, scale=scale)).to(p.device, p.dtype)
        elif name.startswith(("field.mlp", "proposal_fields", "lidar_decoder")) and name.endswith("weight") and p.dim() == 2:
            w, _ = synth.linear(p.shape[0], p.shape[1], 100 + k)
            p.data = T(w).to(p.device)
        elif name.startswith(("field.mlp", "lidar_decoder")) and name.endswith("bias"):
            p.data = T(synth.uniform(tuple(p.shape), -0.2, 0.2, 100 + k)).to(p.device)
    # a translucent static scene (positive SDF offset): the rays reach the actors' corridor 10-25 m out, so that the actor
    # grids and the trajectories receive gradients of the same order as the static table's
    with torch.no_grad():
        model.field.mlp_geo.layers[-1].bias[0] = 1.2
    model.appearance_embedding.weight.data = T(synth.normal(tuple(model.appearance_embedding.weight.shape), seed=77)).to(
        model.appearance_embedding.weight.device)


@pytest.fixture(scope="module")
def ref():
    ref_import.install()
    import nerfstudio.model_components.renderers as ref_renderers
    import nerfstudio.models.neurad as ref_neurad

    saved = (ref_neurad.VGGPerceptualLossPix2Pix, ref_neurad.nerfacc, ref_renderers.nerfacc,
             os.environ.get("NERFSTUDIO_METHOD_CONFIGS"))
    ref_neurad.VGGPerceptualLossPix2Pix = torch.nn.Identity
    os.environ["NERFSTUDIO_METHOD_CONFIGS"] = "neurad-hip=neurad_studio_amd.integration.neurad_hip:neurad_hip"
    yield ref_neurad
    ref_neurad.VGGPerceptualLossPix2Pix, ref_neurad.nerfacc, ref_renderers.nerfacc = saved[:3]
    if saved[3] is None:
        os.environ.pop("NERFSTUDIO_METHOD_CONFIGS", None)
    else:
        os.environ["NERFSTUDIO_METHOD_CONFIGS"] = saved[3]


def shrink(c):
    c.field.grid.static.log2_hashmap_size = 12
    c.field.grid.actor.log2_hashmap_size = 9
    c.field.sdf_beta = 3.0
    for pf in (c.sampling.proposal_field_1, c.sampling.proposal_field_2):
        pf.grid.static.log2_hashmap_size = 10
        pf.grid.actor.log2_hashmap_size = 8
    c.loss.vgg_mult = 0.0
    return c


def build_pair(ref_neurad, with_actors, fused_decoder=False, pose_opt=False, n_actors=3, fp16_tables=False, use_sdf=True,
               normalize_depth=False):
    """(the plugin on cuda:0, resolved through the registry; the reference's torch model on the CPU; same weights).
    pose_opt: camera_optimizer.mode = "SO3xR3" on both (the `*-scaleopt` methods, configs/method_configs.py:438-447), with
    non-zero pose adjustments so that the rays really move.  n_actors > 3: `many_trajectories`.  fp16_tables: the plugin's
    main-field static table and actor grids in fp16 STORAGE (BASELINE config[4]); the reference's fp32 tables then hold exactly
    those rounded values"""
    import nerfstudio.model_components.renderers as ref_renderers
    from nerfstudio.data.scene_box import SceneBox

    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModel

    mcfg = shrink(deepcopy(methods()["neurad-hip"].pipeline.model))
    mcfg.fused_decoder = fused_decoder
    if fp16_tables:  # the plugin's own switch (integration/neurad_hip.py: NeuRADHipModelConfig.table_dtype)
        mcfg.table_dtype = "float16"
    mcfg.field.use_sdf, mcfg.normalize_depth = use_sdf, normalize_depth
    if pose_opt:
        mcfg.camera_optimizer = deepcopy(mcfg.camera_optimizer)
        mcfg.camera_optimizer.mode = "SO3xR3"

    def kw():
        return dict(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                    metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"},
                              "trajectories": (trajectories() if n_actors == 3 else many_trajectories(n_actors))
                              if with_actors else []})

    torch.manual_seed(0)
    hip = mcfg.setup(**kw())
    assert isinstance(hip, NeuRADHipModel) and isinstance(hip, ref_neurad.NeuRADModel), type(hip).__mro__
    ref_cfg = shrink(ref_neurad.NeuRADModelConfig(implementation="torch"))
    for c in (ref_cfg.field, ref_cfg.sampling.proposal_field_1, ref_cfg.sampling.proposal_field_2):
        c.grid.actor.use_4d_hashgrid = False
    if pose_opt:  # (the method table's camera optimizer carries its own penalties: the same object on both sides)
        ref_cfg.camera_optimizer = deepcopy(mcfg.camera_optimizer)
    ref_cfg.field.use_sdf, ref_cfg.normalize_depth = use_sdf, normalize_depth
    refm = ref_cfg.setup(**kw())
    assert sorted(hip.state_dict()) == sorted(refm.state_dict()), set(hip.state_dict()) ^ set(refm.state_dict())
    fill(hip)
    if pose_opt:
        pa = hip.camera_optimizer.pose_adjustment
        pa.data = T(synth.normal(tuple(pa.shape), seed=55) * np.float32(0.02)).to(pa.device)
    if fp16_tables:
        grids = [hip.field.hashgrid.static_grid, *hip.field.hashgrid.actor_grids]
        assert all(gr.hash_table.dtype == torch.float16 for gr in grids), [gr.hash_table.dtype for gr in grids]
    refm.load_state_dict({k: (v.float() if v.dtype == torch.float16 else v) for k, v in hip.state_dict().items()})
    hip = hip.to("cuda")
    # the reference on the CPU: dense nerfacc formulas instead of its 0.5 placeholder (models/neurad.py:713-715)
    na = dense_nerfacc()
    ref_neurad.nerfacc = na
    ref_renderers.nerfacc = na
    # (on the INSTANCE: the plugin class inherits from NeuRADModel and must keep the reference's method)
    if use_sdf:
        refm._render_weights = lambda outputs, rs: na.render_weight_from_alpha(
            outputs[ref_neurad.FieldHeadNames.ALPHA].squeeze(-1))[0]
    else:  # models/neurad.py:718-723
        refm._render_weights = lambda outputs, rs: na.render_weight_from_density(
            t_starts=rs.frustums.starts.squeeze(-1), t_ends=rs.frustums.ends.squeeze(-1),
            sigmas=outputs[ref_neurad.FieldHeadNames.DENSITY].squeeze(-1))[0]
    return hip, refm


def batch(with_actors, patch=4, n_patches=3, n_lidar=40, n_actors=3):
    """camera rays in ``patch`` x ``patch`` patches (the CNN decoder's unit) then lidar rays; with actors the rays are
    aimed down the actors' corridor so that many samples fall inside boxes"""
    Rc = n_patches * patch * patch
    R = Rc + n_lidar
    o = synth.normal((R, 3), 5) * np.array([1.5, 1.5, 0.3], np.float32)
    if with_actors:
        if n_actors == 3:
            tgt = np.stack([synth.uniform((R,), 10, 24, 8),
                            np.where(np.arange(R) % 2 == 0, 8.0, -5.5) + synth.uniform((R,), -1.5, 1.5, 9),
                            synth.uniform((R,), 0.0, 1.0, 10)], -1).astype(np.float32)
        else:  # down the two lanes of `many_trajectories`: shallow angles, several boxes along a ray
            tgt = np.stack([synth.uniform((R,), 12, 8.0 + 3.0 * n_actors, 28),
                            np.where(np.arange(R) % 2 == 0, 6.5, -5.5) + synth.uniform((R,), -1.0, 1.0, 9),
                            synth.uniform((R,), 0.1, 0.9, 10)], -1).astype(np.float32)
        d = tgt - o
    else:
        d = synth.normal((R, 3), 6)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    is_lidar = np.arange(R) >= Rc
    did_return = np.where(is_lidar, synth.uniform((R,), 0, 1, 7) < 0.75, True)
    dist = synth.uniform((R,), 6.0, 40.0, 8)
    area = np.where(is_lidar, 4.5e-6, 2.7e-7).astype(np.float32)
    times = synth.uniform((R,), 0.2, 3.8, 9)
    sensor = np.where(is_lidar, 2, (np.arange(R) // (patch * patch)) % 2).astype(np.int64)
    up = 3 * patch
    image = synth.uniform((n_patches, up, up, 3), 0.0, 1.0, 31)
    lidar = np.concatenate([synth.normal((n_lidar, 3), 21), synth.uniform((n_lidar, 1), 0, 1, 22)], -1)
    return dict(o=o, d=d, is_lidar=is_lidar, did_return=did_return, dist=dist, area=area, times=times, sensor=sensor,
                image=image, lidar=lidar, patch=patch, Rc=Rc)


def bundle(b, device):
    from nerfstudio.cameras.rays import RayBundle

    t = lambda a: T(a).to(device)  # noqa: E731
    return RayBundle(origins=t(b["o"]), directions=t(b["d"]), pixel_area=t(b["area"])[:, None], times=t(b["times"])[:, None],
                     camera_indices=(torch.arange(len(b["o"]), device=device) % 2)[:, None],
                     metadata={"is_lidar": torch.from_numpy(b["is_lidar"])[:, None].to(device),
                               "did_return": torch.from_numpy(b["did_return"])[:, None].to(device),
                               "directions_norm": t(b["dist"])[:, None],
                               "sensor_idxs": torch.from_numpy(b["sensor"])[:, None].to(device)})


def labels(b, device):
    return {"image": T(b["image"]).to(device), "lidar": T(b["lidar"]).to(device),
            "is_lidar": torch.from_numpy(b["is_lidar"])[:, None].to(device),
            "did_return": torch.from_numpy(b["did_return"])[:, None].to(device),
            "distance": T(b["dist"][b["is_lidar"]])[:, None].to(device)}


def deterministic(m, train):
    m.train(train)
    m.sampler.eval(), m.field.eval()
    for p in m.proposal_fields:
        p.eval()
    return m


def losses(m, b, device):
    m.zero_grad(set_to_none=True)
    outputs = m.get_outputs(bundle(b, device), patch_size=(b["patch"], b["patch"]), calc_lidar_losses=True)
    lab = labels(b, device)
    metrics = m.get_metrics_dict(outputs, lab)
    return outputs, m.get_loss_dict(outputs, lab, metrics)


def kind(name):
    if name.endswith("hash_table"):
        return "actor_grid" if "actor_grids" in name else "table"
    if name.startswith("dynamic_actors"):
        return "trajectory"
    if name.startswith("camera_optimizer"):
        return "pose"
    if name.startswith("rgb_decoder"):
        return "decoder"
    if name.startswith("lidar_decoder"):
        return "lidar_head"
    if name.startswith("appearance_embedding"):
        return "embedding"
    if name.endswith("sdf_to_density.beta"):
        return "beta"
    return "mlp"


def analytically_zero(name):
    """convolution biases that feed a BatchNorm: their gradient is zero in exact arithmetic (rounding noise in fp32)"""
    return name.startswith("rgb_decoder") and name.endswith((".main_branch.0.bias", ".main_branch.3.bias"))


OUTLIER_REL = 1e-4


def outlier_stats(a, c, by_rows):
    """(# units of ``a`` further than OUTLIER_REL x the largest unit of ``c`` from ``c``, # units ``c`` reaches, squared error
    and squared norm over the REST).  Unit = a table row (hash tables: a ReLU-kink flip switches one sample's 8 corners x L
    levels on or off) or an element (everything else)."""
    a, c = a.detach().double().cpu(), c.detach().double().cpu()
    if by_rows:
        diff, mag = (a - c).norm(dim=-1), c.norm(dim=-1)
    else:
        diff, mag = (a - c).abs().reshape(-1), c.abs().reshape(-1)
    out = diff > OUTLIER_REL * float(mag.max())
    reached = mag > 0
    rest = ~out
    return int(out.sum()), int(reached.sum()), float((diff[rest] ** 2).sum()), float((mag[rest] ** 2).sum())


def per_loss_gradient_errors(got_model, got_losses, want_model, want_losses, detail=False):
    """{loss term: {parameter kind: worst rel-L2 over the kind's tensors of d loss / d parameter}} of ``got`` against
    ``want``, one backward per term of get_loss_dict on either side (also used by oracle/grad_noise_floor.py: the
    reference in fp32 against itself in fp64).  detail=True: {term: {kind: {"rel_l2", "outlier_frac" (units further than
    1e-4 of the tensor's largest unit from the reference / units the reference reaches), "rest_rel_l2" (over the other
    units, pooled over the kind's tensors)}}} -- what separates "a few ReLU-kink flips" from "a wrong gradient"."""
    names = [n for n, p in want_model.named_parameters() if p.requires_grad and not analytically_zero(n)]
    gp, wp = dict(got_model.named_parameters()), dict(want_model.named_parameters())
    res = {}
    for term in want_losses:
        gg = torch.autograd.grad(got_losses[term], [gp[n] for n in names], retain_graph=True, allow_unused=True)
        wg = torch.autograd.grad(want_losses[term], [wp[n] for n in names], retain_graph=True, allow_unused=True)
        tot = {}
        for n, c in zip(names, wg):
            if c is not None:
                tot[kind(n)] = max(tot.get(kind(n), 0.0), float(c.double().norm()))
        worst, pooled = {}, {}
        for n, a, c in zip(names, gg, wg):
            k = kind(n)
            # a tensor this term barely reaches (1e-6 of its kind's largest gradient) carries rounding noise only
            if c is None or float(c.double().norm()) <= 1e-6 * tot[k]:
                continue
            assert a is not None, f"{term}: {n} has a gradient on the reference side and none on the other"
            if a.dtype == torch.float16:  # fp16-storage table: autograd hands the parameter an fp16 gradient -- held to
                c = c.half().float()       # the fp16 ROUNDING of the reference's gradient (what that storage can express)
            e = float((a.detach().double().cpu() - c.detach().double().cpu()).norm() / c.detach().double().norm())
            worst[k] = max(worst.get(k, 0.0), e)
            if detail:
                st = outlier_stats(a, c, by_rows=k in ("table", "actor_grid"))
                pooled[k] = [x + y for x, y in zip(pooled.get(k, [0, 0, 0.0, 0.0]), st)]
        if detail:
            res[term] = {k: {"rel_l2": worst[k], "outlier_frac": pooled[k][0] / max(pooled[k][1], 1),
                             "n_outliers": pooled[k][0], "n_units": pooled[k][1],
                             "rest_rel_l2": (pooled[k][2] / max(pooled[k][3], 1e-300)) ** 0.5} for k in worst}
        else:
            res[term] = worst
    return res


def floors(scene):
    """the reference's own fp32 noise floor per (loss term, parameter kind): oracle/grad_noise_floor.py ->
    profiles/r05_grad_noise_floor.json = {scene: {"fp32_vs_fp64": detail, "perturbed_max": detail}}"""
    import json

    f = os.path.join(ROOT, "profiles", "r05_grad_noise_floor.json")
    return json.load(open(f))[scene]


def check_gradients_against_floor(errs, floors, report_name=None):
    """Every (loss term, parameter kind) against THAT term's and kind's floor -- the reference's own noise: the larger of its
    fp32-vs-fp64 rel-L2 and of its rel-L2 against itself with inputs perturbed at the fp32 rounding level (the maximum over
    ``perturbed_trials`` draws; the noise is heavy-tailed: a ReLU-kink flip of one hidden unit switches one sample's whole
    contribution on or off, and the two yardsticks differ by up to 6 x on the lidar terms).  Passes when
      rel-L2 <= max(3 x floor, 1e-4),
    or, failing that, when the difference looks like the reference's own noise and like nothing else: at most 2 x (+ 2) as
    many units (table rows / elements) further than 1e-4 of the tensor's largest unit from the reference as the reference
    shows against itself, and over all OTHER units a rel-L2 <= max(2e-4, 2 x the reference's own over its other units).
    -> report {term/kind: {...}}, written to gpurun_out/ when ``report_name`` is given."""
    f64, pert = floors["fp32_vs_fp64"], floors["perturbed_max"]
    zero = {"rel_l2": 0.0, "outlier_frac": 0.0, "rest_rel_l2": 0.0}
    report, bad = {}, []
    for term, kinds in errs.items():
        for kind, st in kinds.items():
            fl = f64.get(term, {}).get(kind, zero)
            pt = pert.get(term, {}).get(kind, zero)
            floor = max(fl["rel_l2"], pt["rel_l2"])
            tol = max(3.0 * floor, 1e-4)
            ref_frac = max(fl["outlier_frac"], pt["outlier_frac"])
            ref_rest = max(fl["rest_rel_l2"], pt["rest_rel_l2"])
            ok_direct = st["rel_l2"] <= tol
            ok_flips = (st["n_outliers"] <= 2.0 * ref_frac * st["n_units"] + 2
                        and st["rest_rel_l2"] <= max(2e-4, 2.0 * ref_rest))
            report[f"{term}/{kind}"] = dict(
                rel_l2=float(f"{st['rel_l2']:.2e}"), bound=float(f"{tol:.2e}"), within_bound=ok_direct,
                outlier_frac=float(f"{st['outlier_frac']:.2e}"), n_outliers=st["n_outliers"], n_units=st["n_units"],
                rest_rel_l2=float(f"{st['rest_rel_l2']:.2e}"),
                reference_fp32_vs_fp64={k: float(f"{fl[k]:.2e}") for k in zero},
                reference_perturbed_max={k: float(f"{pt[k]:.2e}") for k in zero})
            if not (ok_direct or ok_flips):
                bad.append((term, kind, report[f"{term}/{kind}"]))
    if report_name and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        import json

        json.dump(report, open(os.path.join(ROOT, "gpurun_out", report_name), "w"), indent=1)
    assert not bad, bad
    return report


# ---- the reference's own training loop (engine/trainer.py:535-579) around a model ---------------------------------------
K = 10


def batch_k(with_actors, k, n_actors=3):
    """iteration k's batch: the test scene's rays moved a little further along each iteration, labels rolled"""
    b = batch(with_actors, n_actors=n_actors)
    b = dict(b)
    b["o"] = (b["o"] + np.float32(0.15 * k) * np.array([1.0, -0.5, 0.02], np.float32)).astype(np.float32)
    b["times"] = (0.2 + (b["times"] - 0.2 + 0.31 * k) % 3.6).astype(np.float32)
    b["image"] = np.roll(b["image"], k, axis=1)
    b["lidar"] = np.roll(b["lidar"], k, axis=0)
    b["dist"] = (6.0 + (b["dist"] - 6.0 + 1.7 * k) % 34.0).astype(np.float32)
    return b


class Pipeline:
    """what ``ADPipeline.get_train_loss_dict`` (pipelines/ad_pipeline.py:78-100 -- the reference's method, called unbound)
    reads from its pipeline: a datamanager that hands out (ray_bundle, batch), the model, config.ray_patch_size"""

    def __init__(self, model, with_actors, device, dtype, n_actors=3):
        self._model = self.model = model
        self.config = types.SimpleNamespace(ray_patch_size=None)
        self.datamanager = types.SimpleNamespace(next_train=self._next_train)
        self._args = (with_actors, device, dtype, n_actors)

    def _next_train(self, step):
        with_actors, device, dtype, n_actors = self._args
        b = batch_k(with_actors, step, n_actors)
        self.config.ray_patch_size = (b["patch"], b["patch"])
        rb, lab = bundle(b, device), labels(b, device)
        if dtype == torch.float64:
            for k in ("origins", "directions", "pixel_area", "times"):
                setattr(rb, k, getattr(rb, k).double())
            rb.metadata["directions_norm"] = rb.metadata["directions_norm"].double()
            lab = {k: (v.double() if v.is_floating_point() else v) for k, v in lab.items()}
        return rb, lab

    def get_train_loss_dict(self, step):
        from nerfstudio.pipelines.ad_pipeline import ADPipeline

        return ADPipeline.get_train_loss_dict(self, step)


class Loop:
    """the attributes ``Trainer.train_iteration`` reads (engine/trainer.py:176-189,535-579), set as ``Trainer.__init__`` /
    ``Trainer.setup`` set them; the iteration itself is the reference's own function"""

    def __init__(self, method_config, model, pipeline, device, mixed_precision, warmup=True):
        from nerfstudio.engine.optimizers import Optimizers
        from torch.cuda.amp.grad_scaler import GradScaler  # engine/trainer.py:40

        self.config = types.SimpleNamespace(log_gradients=False)
        self.device = device
        self.mixed_precision = bool(mixed_precision) and not device.startswith("cpu")
        self.grad_scaler = GradScaler(enabled=self.mixed_precision)
        self.gradient_accumulation_steps = defaultdict(lambda: 1)
        self.pipeline = pipeline
        # Trainer.setup_optimizers (engine/trainer.py:264-275): the method's optimizer table x the model's parameter groups
        groups = {k: v for k, v in model.get_param_groups().items() if len(v)}
        table = deepcopy({k: method_config.optimizers[k] for k in groups})
        if not warmup:  # full learning rates from the first iteration (the shipped schedules ramp up over 500 - 2500 steps:
            for v in table.values():  # ten iterations of those move the parameters by 1e-4 only)
                v["scheduler"].warmup_steps = 0
        self.optimizers = Optimizers(table, groups)

    def run(self, n):
        from nerfstudio.engine.trainer import Trainer

        losses = []
        for step in range(n):
            _, loss_dict, _ = Trainer.train_iteration(self, step)
            losses.append({k: float(v) for k, v in loss_dict.items()})
            self.pipeline.model.sampler.step_cb(step)  # the model's AFTER_TRAIN_ITERATION callback (models/neurad.py:291-300)
        return losses


def methods():
    """the reference's method table with ``neurad-hip`` in it.  What ns-train does: importing the table runs the plugin
    discovery (configs/method_configs.py -> plugins/registry.py:56-73, the NERFSTUDIO_METHOD_CONFIGS form); where the table was
    imported earlier in this process, before the variable was set, the discovery is run again"""
    import nerfstudio.configs.method_configs as ref_methods
    from nerfstudio.plugins.registry import discover_methods

    table = dict(ref_methods.all_methods)
    if "neurad-hip" not in table:
        table.update(discover_methods()[0])
    return table


# ---- the synthetic drive: a dataparser that feeds the method's pipeline as PandaSet would --------------------------------
H, W, N_CAM, N_LIDAR, PTS = 48, 72, 3, 2, 700


def poses(n, seed):
    out = []
    for i in range(n):
        yaw = 0.2 * i + 0.05 * float(synth.normal((1,), seed + i)[0])
        c, s = np.cos(yaw), np.sin(yaw)
        # camera looking along +x of the world: columns = (right, up, back)
        rot = np.array([[s, 0.0, -c], [-c, 0.0, -s], [0.0, 1.0, 0.0]], np.float32)
        out.append(np.concatenate([rot, np.array([[2.0 * i], [0.3 * i], [1.6]], np.float32)], 1))
    return np.stack(out).astype(np.float32)


def make_parser_classes(root: Path):
    from nerfstudio.cameras.cameras import Cameras, CameraType
    from nerfstudio.cameras.lidars import Lidars, LidarType
    from nerfstudio.data.dataparsers.base_dataparser import DataParser, DataParserConfig, DataparserOutputs
    from nerfstudio.data.scene_box import SceneBox
    from PIL import Image

    files = []
    for i in range(N_CAM):
        img = (synth.uniform((H, W, 3), 0, 1, 300 + i) * 255).astype(np.uint8)
        f = root / f"cam{i}.png"
        Image.fromarray(img).save(f)
        files.append(f)

    @dataclass
    class SynthParserConfig(DataParserConfig):
        _target: Type = field(default_factory=lambda: SynthParser)
        data: Path = root
        add_missing_points: bool = True  # (read by ADPipeline.__init__, pipelines/ad_pipeline.py:71-73)

    class SynthParser(DataParser):
        includes_time = True

        def _generate_dataparser_outputs(self, split="train", **kwargs):
            md = {"rolling_shutter_time": T(synth.uniform((N_CAM, 1), 0.01, 0.03, 6)),
                  "time_to_center_pixel": T(synth.uniform((N_CAM, 1), -0.01, 0.01, 7)),
                  "velocities": T(synth.normal((N_CAM, 3), 8) * 3), "sensor_idxs": torch.arange(N_CAM)[:, None] % 2}
            cams = Cameras(camera_to_worlds=T(poses(N_CAM, 10)), fx=T(synth.uniform((N_CAM, 1), 60, 70, 1)),
                           fy=T(synth.uniform((N_CAM, 1), 60, 70, 2)), cx=float(W / 2), cy=float(H / 2), width=W, height=H,
                           camera_type=CameraType.PERSPECTIVE, times=T(synth.uniform((N_CAM, 1), 0.3, 3.5, 5)), metadata=md)
            l2w = poses(N_LIDAR, 40)
            lid = Lidars(lidar_to_worlds=T(l2w), lidar_type=LidarType.VELODYNE64E, assume_ego_compensated=True,
                         times=T(synth.uniform((N_LIDAR, 1), 0.3, 3.5, 41)),
                         metadata={"velocities": T(synth.normal((N_LIDAR, 3), 42) * 3),
                                   "sensor_idxs": torch.full((N_LIDAR, 1), 2)}, valid_lidar_distance_threshold=1000.0)
            clouds = []
            for i in range(N_LIDAR):
                p = np.concatenate([synth.normal((PTS, 3), 44 + i) * np.array([15.0, 15.0, 1.0], np.float32),
                                    synth.uniform((PTS, 1), 0, 1, 46 + i), synth.uniform((PTS, 1), -0.05, 0.05, 48 + i)], -1)
                p[:40, :3] *= 200.0  # beams without a return
                clouds.append(T(p))
            return DataparserOutputs(
                image_filenames=list(files), cameras=cams,
                scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])),
                metadata={"lidars": lid, "point_clouds": clouds, "trajectories": trajectories(), "duration": 5.0,
                          "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}})

    return SynthParserConfig


def method_config(tmp_path):
    """the ``neurad-hip`` method's trainer config, pointed at the synthetic drive and shrunk to test size"""
    cfg = deepcopy(methods()["neurad-hip"])
    pc = cfg.pipeline
    pc.ray_patch_size = (4, 4)
    pc.datamanager.dataparser = make_parser_classes(tmp_path)()
    pc.datamanager.train_num_rays_per_batch = 5 * 16
    pc.datamanager.train_num_lidar_rays_per_batch = 48
    pc.datamanager.eval_num_rays_per_batch = 16
    pc.datamanager.eval_num_lidar_rays_per_batch = 16
    pc.datamanager.pixel_sampler.patch_size, pc.datamanager.pixel_sampler.patch_scale = 4, pc.model.rgb_upsample_factor
    shrink(pc.model)
    pc.__post_init__()
    return cfg
