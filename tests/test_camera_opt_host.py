"""Camera pose correction on the CPU: the arithmetic plan of csrc/pose_opt.hip's backward (tests/camera_opt_refs.py emulates its
integer sums) against float64 autograd of the restated formula, its exactness properties, the closed form of the chain the
finish pass evaluates, and the glue of cameras/camera_optimizers.py:CameraOptimizer -- against a stand-in with the reference
module's attributes and, where the reference tree is importable, against the reference's own CameraOptimizer and
ScaledCameraOptimizer.  The kernels themselves: tests/test_gpu_camera_opt.py."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import camera_opt_refs as R  # noqa: E402
import ref_import  # noqa: E402
from conftest import rel_l2  # noqa: E402

from neurad_studio_amd.cameras.camera_optimizers import (METRIC_KEYS, CameraOptimizer, CameraOptimizerConfig,  # noqa: E402
                                                         exp_map_so3xr3)

CASES = R.case_list()


def _emulated(c):
    em = R.emulate_sums(c["idx"], c["d"], c["g_o"], c["g_d"], c["C"])
    return em, R.finish_autograd(c["pose"], c["weights"], em["S"], em["flag"])


@pytest.mark.parametrize("spec", CASES, ids=R.case_id)
def test_integer_sums_meet_the_backward_bound(spec):
    """|g - g64| <= 2^-22 |g64| + 16 n_c 2^-B m_c |w_k| per camera and component; cameras without a ray are exactly zero"""
    c = R.case(*spec)
    em, g = _emulated(c)
    g64 = R.pose_grad64(c["pose"], c["weights"], c["idx"], c["d"], c["g_o"], c["g_d"])
    bound = R.grad_bound(g64, em["n"], em["m"], em["B"], c["weights"])
    err = (g.double() - g64).abs()
    share = float((err / bound.clamp_min(1e-300)).max())
    print("largest share of the bound:", share)
    assert bool((err <= bound).all()), share
    assert bool((g[em["n"] == 0] == 0).all()) and bool((g64[em["n"] == 0] == 0).all())
    # the closed form the finish pass evaluates is the same chain
    gc = R.finish_closed_form(c["pose"], c["weights"], em["S"], em["flag"])
    assert bool(((gc.double() - g64).abs() <= bound).all())
    assert bool(((gc.double() - g.double()).abs() <= 2.0 ** -23 * g.double().abs() + 1e-300).all())


def test_fp32_summation_does_not_fit_the_bound_at_1024_rays_per_camera():
    """what the integer sums are for: the same terms added in fp32 in ray order miss the bound at n_c = 1024"""
    c = R.case(1025, 1, "one", 0.1, False)
    em = R.emulate_sums(c["idx"], c["d"], c["g_o"], c["g_d"], 1)
    terms = torch.from_numpy(R.ray_terms(c["d"], c["g_o"], c["g_d"])).float()
    s32 = torch.zeros(12)
    for row in terms:
        s32 = s32 + row
    g32 = R.finish_autograd(c["pose"], None, s32.double()[None], em["flag"])
    g64 = R.pose_grad64(c["pose"], None, c["idx"], c["d"], c["g_o"], c["g_d"])
    assert not bool(((g32.double() - g64).abs() <= R.grad_bound(g64, em["n"], em["m"], em["B"], None)).all())


@pytest.mark.parametrize("spec", [s for s in CASES if s[0] >= 256][::3], ids=R.case_id)
def test_power_of_two_scaling_and_permutations_are_exact(spec):
    c = R.case(*spec)
    em, g = _emulated(c)
    for k in (16, -20):
        em2 = R.emulate_sums(c["idx"], c["d"], c["g_o"] * 2.0 ** k, c["g_d"] * 2.0 ** k, c["C"])
        assert np.array_equal(em2["q_sums"], em["q_sums"])
        g2 = R.finish_autograd(c["pose"], c["weights"], em2["S"], em2["flag"])
        assert torch.equal(g2, g * 2.0 ** k)
    perm = torch.randperm(c["R"], generator=torch.Generator().manual_seed(3))
    emp = R.emulate_sums(c["idx"][perm], c["d"][perm], c["g_o"][perm], c["g_d"][perm], c["C"])
    assert np.array_equal(emp["q_sums"], em["q_sums"]) and torch.equal(emp["m"], em["m"])


def test_a_camera_with_tiny_terms_keeps_full_precision():
    """terms of camera 5 are 2^-30 of the others': a per-camera scale, so its row is as accurate as every other one"""
    c = R.case(1025, 70, "random", 0.1, True)
    tiny = c["idx"] == 5
    assert int(tiny.sum()) > 3
    c["g_o"][tiny] *= 2.0 ** -30
    c["g_d"][tiny] *= 2.0 ** -30
    em, g = _emulated(c)
    g64 = R.pose_grad64(c["pose"], c["weights"], c["idx"], c["d"], c["g_o"], c["g_d"])
    assert float(em["m"][5]) < 2.0 ** -25 * float(em["m"].max())
    assert bool(((g.double() - g64).abs() <= R.grad_bound(g64, em["n"], em["m"], em["B"], c["weights"])).all())
    rel = ((g.double() - g64).abs()[5] / g64.abs()[5]).max()
    assert float(rel) <= 2.0 ** -22, float(rel)


def test_non_finite_gradients_flag_their_camera_only():
    c = R.case(257, 70, "random", 0.1, False)
    clean = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    c["g_o"][10, 1], c["g_d"][200, 0] = float("inf"), float("nan")
    clean["g_o"][10], clean["g_d"][10], clean["g_o"][200], clean["g_d"][200] = 0.0, 0.0, 0.0, 0.0
    (em, g), (_, gz) = _emulated(c), _emulated(clean)
    bad = {int(c["idx"][10]), int(c["idx"][200])}
    for cam in range(70):
        if cam in bad:
            assert bool(torch.isnan(g[cam]).all())
        else:
            assert torch.equal(g[cam], gz[cam])


# ---- the module ---------------------------------------------------------------------------------------------------------------
class _ReferenceLike(torch.nn.Module):
    """the attributes CameraOptimizer.from_reference reads from the reference's module"""

    def __init__(self, mode, n, weights=None, non_trainable=None, trans=1e-2):
        super().__init__()
        self.config = types.SimpleNamespace(mode=mode, trans_l2_penalty=trans, rot_l2_penalty=1e-3)
        self.num_cameras, self.device, self.non_trainable_camera_indices = n, "cpu", non_trainable
        if mode != "off":
            self.pose_adjustment = torch.nn.Parameter(torch.randn(n, 6, generator=torch.Generator().manual_seed(4)) * 0.05)
        if weights is not None:
            self.register_buffer("weights", torch.tensor(weights, dtype=torch.float32))


def test_from_reference_adopts_the_parameter_and_keeps_the_names():
    for weights in (None, R.SCALED_WEIGHTS):
        module = _ReferenceLike("SO3xR3", 9, weights, trans=(1e-2, 2e-2, 3e-2) if weights else 1e-2)
        ours = CameraOptimizer.from_reference(module)
        assert type(ours) is CameraOptimizer and ours.pose_adjustment is module.pose_adjustment
        assert list(ours.state_dict()) == list(module.state_dict()) == ["pose_adjustment"] + (["weights"] if weights else [])
        if weights:
            assert ours.weights is module.weights
        assert CameraOptimizer.from_reference(ours) is ours
        groups = {}
        ours.get_param_groups(groups)
        assert list(groups) == ["camera_opt"] and groups["camera_opt"][0] is module.pose_adjustment
        ours.load_state_dict(module.state_dict())
    for module in (_ReferenceLike("off", 3), _ReferenceLike("SE3", 3), _ReferenceLike("SO3xR3", 3, non_trainable=torch.tensor([1]))):
        assert CameraOptimizer.from_reference(module) is module


@pytest.mark.parametrize("scaled", [False, True])
def test_metrics_and_regularisers_match_the_restatement(scaled):
    trans = (1e-2, 2e-2, 3e-2) if scaled else 1e-2
    co = CameraOptimizer(CameraOptimizerConfig(trans_l2_penalty=trans, weights=R.SCALED_WEIGHTS if scaled else None), 11)
    with torch.no_grad():
        co.pose_adjustment.copy_(torch.randn(11, 6, generator=torch.Generator().manual_seed(5)) * 0.1)
    p = co.pose_adjustment.detach().double()
    metrics = {}
    co.get_metrics_dict(metrics)
    assert tuple(sorted(metrics)) == tuple(sorted(METRIC_KEYS))
    tn, rn = p[:, :3].norm(dim=-1), p[:, 3:].norm(dim=-1)
    want = {"camera_opt_translation_max": tn.max(), "camera_opt_translation_mean": tn.mean(),
            "camera_opt_rotation_mean": rn.mean() * 180 / math.pi, "camera_opt_rotation_max": rn.max() * 180 / math.pi}
    for k, v in metrics.items():
        assert isinstance(v, torch.Tensor) and v.shape == () and not v.requires_grad and v.device == co.pose_adjustment.device
        assert abs(float(v) - float(want[k])) <= 1e-6 * float(want[k]), k
    loss = {}
    co.get_loss_dict(loss)
    a = p * torch.tensor(R.SCALED_WEIGHTS, dtype=torch.float64) if scaled else p
    rot = a[:, 3:].norm(dim=-1).mean() * 1e-3
    reg = (a[:, :3].abs() * torch.tensor(trans, dtype=torch.float64)).mean() + rot if scaled else tn.mean() * 1e-2 + rot
    assert list(loss) == ["camera_opt_regularizer"] and loss["camera_opt_regularizer"].requires_grad
    assert abs(float(loss["camera_opt_regularizer"]) - float(reg)) <= 1e-6 * float(reg)


@pytest.mark.parametrize("scaled", [False, True])
def test_cpu_path_is_the_restated_formula(scaled):
    """matrices and corrected rays of the CPU path against the helper's float64 restatement, at fp32 rounding level; one ray
    keeps its [1, 3] shape"""
    c = R.case(257, 70, "random", 0.1, scaled)
    co = CameraOptimizer(CameraOptimizerConfig(weights=R.SCALED_WEIGHTS if scaled else None), 70)
    with torch.no_grad():
        co.pose_adjustment.copy_(c["pose"])
    Rm, t = R.exp_map(R.tangent(c["pose"], c["weights"], torch.float64)[c["idx"]])
    m = co(c["idx"])
    assert m.shape == (257, 3, 4) and torch.equal(co.get_correction_matrices(), co(torch.arange(70)))
    assert float((m[:, :, :3].double() - Rm).abs().max()) <= 8 * R.U and float((m[:, :, 3].double() - t).abs().max()) <= R.U
    rb = types.SimpleNamespace(origins=c["o"].clone(), directions=c["d"].clone(), camera_indices=c["idx"][:, None])
    co.apply_to_raybundle(rb)
    o64, d64 = R.pose_apply(c["pose"], c["weights"], c["idx"], c["o"], c["d"])
    bo, bd = R.forward_bounds(c["pose"], c["weights"], c["idx"], c["o"], c["d"])
    assert rb.origins.requires_grad and bool(((rb.origins.double() - o64).abs() <= bo).all())
    assert bool(((rb.directions.double() - d64).abs() <= bd).all())
    one = types.SimpleNamespace(origins=c["o"][:1].clone(), directions=c["d"][:1].clone(), camera_indices=c["idx"][:1, None])
    co.apply_to_raybundle(one)
    assert one.origins.shape == one.directions.shape == (1, 3)
    assert torch.equal(exp_map_so3xr3(torch.zeros(2, 6))[:, :, :3], torch.eye(3).expand(2, 3, 3))


@pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
@pytest.mark.parametrize("scaled", [False, True])
def test_cpu_path_equals_the_reference_modules(scaled):
    """fp32 against fp32: matrices, corrected rays and the loss-dict entry of the reference's CameraOptimizer /
    ScaledCameraOptimizer and of this package's module around the same parameter -- rel-L2 below 1e-4 and 1e-4 relative, the
    tolerances of the plugin-host tests' torch-against-torch comparisons (tests/test_lidar_eval_plugin_host.py)"""
    ref_import.install()
    from nerfstudio.cameras import camera_optimizers as ref_co
    from nerfstudio.cameras.rays import RayBundle

    if scaled:
        cfg = ref_co.ScaledCameraOptimizerConfig(mode="SO3xR3", weights=R.SCALED_WEIGHTS, trans_l2_penalty=(1e-2, 2e-2, 3e-2))
    else:
        cfg = ref_co.CameraOptimizerConfig(mode="SO3xR3")
    module = cfg.setup(num_cameras=70, device="cpu")
    c = R.case(257, 70, "random", 0.1, scaled)
    with torch.no_grad():
        module.pose_adjustment.copy_(c["pose"])
    ours = CameraOptimizer.from_reference(module)
    assert type(ours) is CameraOptimizer and ours.pose_adjustment is module.pose_adjustment
    assert list(ours.state_dict()) == list(module.state_dict())
    assert rel_l2(ours(c["idx"]).detach(), module(c["idx"]).detach()) < 1e-4

    def bundle():
        return RayBundle(origins=c["o"].clone(), directions=c["d"].clone(), pixel_area=torch.ones(257, 1),
                         camera_indices=c["idx"][:, None])

    a, b = bundle(), bundle()
    ours.apply_to_raybundle(a), module.apply_to_raybundle(b)
    assert a.origins.shape == b.origins.shape and a.directions.shape == b.directions.shape
    assert rel_l2(a.origins.detach(), b.origins.detach()) < 1e-4 and rel_l2(a.directions.detach(), b.directions.detach()) < 1e-4
    la, lb = {}, {}
    ours.get_loss_dict(la), module.get_loss_dict(lb)
    x, y = float(la["camera_opt_regularizer"]), float(lb["camera_opt_regularizer"])
    assert list(la) == list(lb) and abs(x - y) <= 1e-4 * abs(y)
    ma, mb = {}, {}
    ours.get_metrics_dict(ma), module.get_metrics_dict(mb)
    assert list(ma) == list(mb)
    for k in ma:
        assert abs(float(ma[k]) - float(mb[k])) <= 1e-4 * abs(float(mb[k])), k
    # the reference's own classes are handed back where this one does not restate them
    for kw in (dict(mode="off"), dict(mode="SE3")):
        m = ref_co.CameraOptimizerConfig(**kw).setup(num_cameras=3, device="cpu")
        assert CameraOptimizer.from_reference(m) is m
    m = ref_co.CameraOptimizerConfig(mode="SO3xR3").setup(num_cameras=3, device="cpu", non_trainable_camera_indices=torch.tensor([0]))
    assert CameraOptimizer.from_reference(m) is m
