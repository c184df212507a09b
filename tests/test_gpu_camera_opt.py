"""csrc/pose_opt.hip on the GPU: ``ops.pose_apply`` / ``ops.pose_apply_bwd``, ``autograd.PoseApplyFn`` and
cameras/camera_optimizers.py:CameraOptimizer against the float64 restatement of tests/camera_opt_refs.py on the same fp32
inputs, per element within the bounds of include/neurad_hip.h, and the bit-for-bit properties of the backward: two runs, any
permutation of the rays, power-of-two scaling, non-finite gradients, out-of-range indices, graph capture.

Shares of the bounds seen on an MI355X (each test prints its own; the largest over all cases):
forward origins 0.50 and directions 0.33, backward 0.24, input direction gradients 0.38."""
import math
import types

import pytest
import torch

import camera_opt_refs as R

pytestmark = pytest.mark.gpu
CASES = R.case_list()


def dev(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def bwd(g, g_o=None, g_d=None, **kw):
    from neurad_studio_amd import ops

    return ops.pose_apply_bwd(g["pose"], g["weights"], g["idx"], g["d"], g["g_o"] if g_o is None else g_o,
                              g["g_d"] if g_d is None else g_d, **kw)


_cache = {}


def run(spec):
    """one case: (the case on the CPU, on the device, the device forward and backward); computed once, shared, never written"""
    if spec not in _cache:
        from neurad_studio_amd import ops

        c = R.case(*spec)
        g = dev(c)
        _cache[spec] = (c, g, ops.pose_apply(g["pose"], g["weights"], g["idx"], g["o"], g["d"]), bwd(g)[0])
    return _cache[spec]


@pytest.mark.parametrize("spec", CASES, ids=R.case_id)
def test_forward_is_within_its_bounds_of_float64(spec):
    c, g, (o2, d2), _ = run(spec)
    o64, d64 = R.pose_apply(c["pose"], c["weights"], c["idx"], c["o"], c["d"])
    bo, bd = R.forward_bounds(c["pose"], c["weights"], c["idx"], c["o"], c["d"])
    assert o2.shape == d2.shape == (c["R"], 3) and o2.dtype == d2.dtype == torch.float32
    eo, ed = (o2.cpu().double() - o64).abs(), (d2.cpu().double() - d64).abs()
    print("share of the forward bounds (origins, directions):", float((eo / bo.clamp_min(1e-300)).max()), float((ed / bd).max()))
    assert bool((eo <= bo).all()) and bool((ed <= bd).all())


@pytest.mark.parametrize("spec", CASES, ids=R.case_id)
def test_backward_is_within_its_bound_of_float64_autograd(spec):
    c, g, _, gp = run(spec)
    g64 = R.pose_grad64(c["pose"], c["weights"], c["idx"], c["d"], c["g_o"], c["g_d"])
    em = R.emulate_sums(c["idx"], c["d"], c["g_o"], c["g_d"], c["C"])
    bound = R.grad_bound(g64, em["n"], em["m"], em["B"], c["weights"])
    err = (gp.cpu().double() - g64).abs()
    print("share of the backward bound:", float((err / bound.clamp_min(1e-300)).max()))
    assert gp.shape == (c["C"], 6) and bool((err <= bound).all())
    untouched = em["n"] == 0
    assert bool((gp.cpu()[untouched] == 0).all()) and not bool(torch.signbit(gp.cpu()[untouched]).any())
    # the integer sums themselves are what the emulation says: the finish pass's closed form on them, to the last bit but one
    want = R.finish_closed_form(c["pose"], c["weights"], em["S"], em["flag"])
    assert bool(((gp.cpu().double() - want.double()).abs() <= 2.0 ** -22 * want.double().abs()).all())


@pytest.mark.parametrize("spec", CASES, ids=R.case_id)
def test_backward_bits_do_not_depend_on_run_order_or_scale(spec):
    c, g, _, gp = run(spec)
    assert torch.equal(bwd(g)[0], gp)
    gen = torch.Generator().manual_seed(11)
    for _ in range(3):
        perm = torch.randperm(c["R"], generator=gen).cuda()
        p = dict(g, idx=g["idx"][perm], d=g["d"][perm], g_o=g["g_o"][perm], g_d=g["g_d"][perm])
        assert torch.equal(bwd(p)[0], gp)
    for k in (16, -20):
        assert torch.equal(bwd(g, g["g_o"] * 2.0 ** k, g["g_d"] * 2.0 ** k)[0], gp * 2.0 ** k), k


def test_non_finite_gradients_make_their_camera_nan_and_leave_the_others():
    c = R.case(257, 70, "random", 0.1, True)
    g = dev(c)
    g_o, g_d = g["g_o"].clone(), g["g_d"].clone()
    g_o[10, 1], g_d[200, 0] = float("inf"), float("nan")
    z_o, z_d = g["g_o"].clone(), g["g_d"].clone()
    z_o[10], z_d[10], z_o[200], z_d[200] = 0.0, 0.0, 0.0, 0.0
    got, zeroed = bwd(g, g_o, g_d)[0].cpu(), bwd(g, z_o, z_d)[0].cpu()
    bad = {int(c["idx"][10]), int(c["idx"][200])}
    assert len(bad) == 2
    for cam in range(70):
        if cam in bad:
            assert bool(torch.isnan(got[cam]).all()), cam
        else:
            assert torch.equal(got[cam], zeroed[cam]), cam


def test_out_of_range_indices_touch_nothing():
    """indices -1 and C: the parameter, the gradient and the workspace are views with a spare row either side, so that a read
    or write that missed the guard would still land inside an allocation -- and show"""
    from neurad_studio_amd import ops

    C, n = 5, 300
    c = R.case(n, C, "random", 0.1, True)
    keep = torch.ones(n, dtype=torch.bool)
    keep[[17, 130]] = False
    c["idx"][17], c["idx"][130] = -1, C
    g = dev(c)
    big = torch.full((C + 2, 6), 1e3, device="cuda")
    big[1:C + 1] = g["pose"]
    pose = big[1:C + 1]
    assert pose.is_contiguous() and pose.data_ptr() == big.data_ptr() + 24
    o2, d2 = ops.pose_apply(pose, g["weights"], g["idx"], g["o"], g["d"])
    want_o, want_d = ops.pose_apply(g["pose"], g["weights"], g["idx"][keep.cuda()], g["o"][keep.cuda()], g["d"][keep.cuda()])
    assert torch.equal(o2[~keep.cuda()], g["o"][~keep.cuda()]) and torch.equal(d2[~keep.cuda()], g["d"][~keep.cuda()])
    assert torch.equal(o2[keep.cuda()], want_o) and torch.equal(d2[keep.cuda()], want_d)
    # the C entry itself, so that the gradient and the workspace can be views as well
    big_g = torch.full((C + 2, 6), 7.0, device="cuda")
    big_ws = torch.full(((C + 2) * 128,), 0xAB, device="cuda", dtype=torch.uint8)
    gi_o, gi_d = torch.empty_like(g["g_o"]), torch.empty_like(g["g_d"])
    ops.launch("nrhip_pose_apply_bwd", pose, g["weights"], C, g["idx"], g["d"], g["g_o"], g["g_d"], n, big_ws[128:(C + 1) * 128],
               big_g[1:C + 1], gi_o, gi_d)
    k = keep.cuda()
    without = ops.pose_apply_bwd(g["pose"], g["weights"], g["idx"][k], g["d"][k], g["g_o"][k], g["g_d"][k], True, True)
    assert R.bits_B(n) == R.bits_B(int(keep.sum()))  # (the scale of the sums depends on ceil(log2 r): the same for both runs)
    assert torch.equal(big_g[1:C + 1], without[0])
    assert bool((big_g[0] == 7.0).all()) and bool((big_g[C + 1] == 7.0).all())
    assert bool((big_ws[:128] == 0xAB).all()) and bool((big_ws[(C + 1) * 128:] == 0xAB).all())
    assert bool((big[0] == 1e3).all()) and bool((big[C + 1] == 1e3).all()) and torch.equal(big[1:C + 1], g["pose"])
    assert torch.equal(gi_o[k], without[1]) and torch.equal(gi_d[k], without[2])
    assert torch.equal(gi_o[~k], g["g_o"][~k]) and torch.equal(gi_d[~k], g["g_d"][~k])


@pytest.mark.parametrize("spec", [s for s in CASES if s[0] in (65, 1025)], ids=R.case_id)
def test_rays_that_require_grad_get_their_gradients(spec):
    """grad_o_in = g_o exactly; |grad_d_in - float64| <= 16 u ||g_d||_2 per ray (the forward's form of bound: R^T g_d is the
    same product).  Through the autograd node, together with the parameter's gradient."""
    from neurad_studio_amd.autograd import PoseApplyFn

    c, g, _, gp = run(spec)
    pose = g["pose"].clone().requires_grad_(True)
    o, d = g["o"].clone().requires_grad_(True), g["d"].clone().requires_grad_(True)
    o2, d2 = PoseApplyFn.apply(pose, g["weights"], g["idx"], o, d)
    got_p, got_o, got_d = torch.autograd.grad([o2, d2], [pose, o, d], [g["g_o"], g["g_d"]])
    _, want_o, want_d = R.pose_grad64(c["pose"], c["weights"], c["idx"], c["d"], c["g_o"], c["g_d"], need_rays=True)
    assert torch.equal(got_p, gp) and torch.equal(got_o, g["g_o"]) and bool((want_o == c["g_o"].double()).all())
    bound = (16 * R.U * c["g_d"].double().norm(dim=1))[:, None]
    err = (got_d.cpu().double() - want_d).abs()
    print("share of the input-gradient bound:", float((err / bound).max()))
    assert bool((err <= bound).all())
    # only the rays: a frozen parameter
    o2, d2 = PoseApplyFn.apply(g["pose"], g["weights"], g["idx"], o, d)
    only_o, only_d = torch.autograd.grad([o2, d2], [o, d], [g["g_o"], g["g_d"]])
    assert torch.equal(only_o, got_o) and torch.equal(only_d, got_d)


def _module(c, g):
    from neurad_studio_amd.cameras.camera_optimizers import CameraOptimizer, CameraOptimizerConfig

    co = CameraOptimizer(CameraOptimizerConfig(weights=R.SCALED_WEIGHTS if c["scaled"] else None,
                                               trans_l2_penalty=(1e-2, 2e-2, 3e-2) if c["scaled"] else 1e-2), c["C"]).cuda()
    with torch.no_grad():
        co.pose_adjustment.copy_(g["pose"])
    return co


def _bundle(g, n=None):
    return types.SimpleNamespace(origins=g["o"][:n].clone(), directions=g["d"][:n].clone(), camera_indices=g["idx"][:n, None].clone())


def test_module_is_the_node_fp32_under_autocast_and_forward_only_without_grad(monkeypatch):
    from neurad_studio_amd import ops

    spec = (257, 70, "random", 0.1, True)
    c, g, (o2, d2), gp = run(spec)
    co = _module(c, g)
    rb = _bundle(g)
    with torch.autocast("cuda", dtype=torch.float16):
        co.apply_to_raybundle(rb)
    assert rb.origins.dtype == rb.directions.dtype == torch.float32 and rb.origins.requires_grad
    assert torch.equal(rb.origins, o2) and torch.equal(rb.directions, d2)  # directions are NOT rounded through fp16
    got = torch.autograd.grad([rb.origins, rb.directions], [co.pose_adjustment], [g["g_o"], g["g_d"]])[0]
    assert torch.equal(got, gp)
    one = _bundle(g, 1)
    co.apply_to_raybundle(one)
    assert one.origins.shape == one.directions.shape == (1, 3)
    # use_camopt_in_eval: no graph, no backward kernels, no workspace
    calls = []
    monkeypatch.setattr(ops, "_workspace", lambda *a, **k: calls.append("workspace"))
    monkeypatch.setattr(ops, "pose_apply_bwd", lambda *a, **k: calls.append("bwd"))
    rb = _bundle(g)
    with torch.no_grad():
        co.apply_to_raybundle(rb)
    assert calls == [] and rb.origins.grad_fn is None and not rb.directions.requires_grad
    assert torch.equal(rb.origins, o2) and torch.equal(rb.directions, d2)
    # the metrics: device tensors, the restated values
    metrics = {}
    co.get_metrics_dict(metrics)
    rot = c["pose"][:, 3:].double().norm(dim=-1)
    assert all(v.is_cuda and v.shape == () for v in metrics.values()) and len(metrics) == 4
    assert abs(float(metrics["camera_opt_rotation_max"]) - float(rot.max()) * 180 / math.pi) <= 1e-5 * float(rot.max()) * 180 / math.pi


def test_empty_batches_launch_nothing():
    from neurad_studio_amd import ops

    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    idx = torch.zeros(0, dtype=torch.int64, device="cuda")
    pose = torch.randn(4, 6, device="cuda")
    o2, d2 = ops.pose_apply(pose, None, idx, z(0, 3), z(0, 3))
    assert o2.shape == d2.shape == (0, 3)
    gp, gi_o, gi_d = ops.pose_apply_bwd(pose, None, idx, z(0, 3), z(0, 3), z(0, 3), True, True)
    assert torch.equal(gp, torch.zeros_like(pose)) and gi_o.shape == gi_d.shape == (0, 3)
    ops.launch("nrhip_pose_apply", None, None, 0, None, None, None, 5, None, None)  # no camera: nothing is dereferenced
    ops.launch("nrhip_pose_apply_bwd", None, None, 4, None, None, None, None, 0, None, None, None, None)
    with pytest.raises(TypeError):
        ops.pose_apply(pose, None, idx.int(), z(0, 3), z(0, 3))


def test_forward_backward_metrics_and_regulariser_replay_from_a_graph():
    """forward + backward + get_metrics_dict + get_loss_dict captured in one graph (which also shows that none of them reads the
    host or allocates outside torch's pool), replayed twice with new ray gradients copied in: each replay equals the eager
    result bit for bit.  The machine's default queue count."""
    spec = (1025, 70, "runs100", 0.1, True)
    c, g, _, _ = run(spec)
    co = _module(c, g)
    G_o, G_d = g["g_o"].clone(), g["g_d"].clone()

    def step():
        rb = _bundle(g)
        co.apply_to_raybundle(rb)
        gp = torch.autograd.grad([rb.origins, rb.directions], [co.pose_adjustment], [G_o, G_d])[0]
        metrics, loss = {}, {}
        co.get_metrics_dict(metrics), co.get_loss_dict(loss)
        return [rb.origins.detach(), rb.directions.detach(), gp, loss["camera_opt_regularizer"].detach(), *metrics.values()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        G_o.copy_(torch.randn(1025, 3, generator=gen).cuda())
        G_d.copy_((torch.randn(1025, 3, generator=gen) * 30).cuda())
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        for a, b in zip(replayed, step()):
            assert torch.equal(a, b)
