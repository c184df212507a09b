"""The two per-sample loss terms on packed, occupancy-marched samples (csrc/losses.hip: nrhip_packed_distortion_loss,
nrhip_packed_lidar_carving) on the device: against the float64 O(n^2) reference and the reference's own mask
(tests/packed_loss_refs.py, tests/golden/packed_losses.npz) within the bounds stated in include/neurad_hip.h, at the
boundaries of the packed contract, through the public functions and through the fused packed training node."""
import numpy as np
import pytest
import torch

import packed_loss_refs as P
import packed_train_refs as T
from gpu_util import cuda, host, host64, ops, ray_bundle  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu
SPARE = 64  # rows behind the live ones: nothing may be written there
NAN = float("nan")
R_FULL = len(P.COUNTS)  # 24 rays: six full blocks of four
R_PART = R_FULL - 2     # 22 rays: the last block is partial (and the ray of 1000 samples is gone)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def nan_rows(n):
    return torch.full((n + SPARE,), NAN, device="cuda")


@pytest.fixture(scope="module")
def dist():
    """the distortion case on the device with its float64 O(n^2) reference and the scales of the bound, computed once"""
    s, e, w, seg = P.distortion_case()
    n, X, S = P.distortion_scales(s, e, w, seg)
    loss, grad = P.distortion_quadratic(s, e, w, seg)
    return {"host": (s, e, w, seg), "dev": (cuda(s), cuda(e), cuda(w), cuda(seg)), "loss": loss, "grad": grad,
            "loss_bound": P.loss_bound(loss, n, X, S), "grad_bound": P.grad_bound(grad, n, X, S, seg), "n": n}


@pytest.fixture(scope="module")
def carve():
    """the carving case on the device with the reference's mask (the fixture) and the loss / gradient that follow from it"""
    c, g = P.carving_case(), P.gold()
    for k, a in c.items():
        assert np.array_equal(g[f"carve_{k}"], a), k
    out = {"host": c, "mask": g["carve_mask"], "mask_all_returned": g["carve_mask_all_returned"]}
    out["dev"] = {k: cuda(v.view(np.uint8) if v.dtype == np.bool_ else v) for k, v in c.items()}
    out["loss"], out["grad"] = P.carving_loss(c["weights"], out["mask"], c["seg"], c["is_lidar"])
    return out


def launch_distortion(ops, s, e, w, seg, R, M, want_grad=True):
    """the C entry point on the first R rays / M samples, outputs pre-filled with NaN and SPARE rows longer"""
    loss, grad = nan_rows(R), nan_rows(M)
    live = lambda t: t if M else None  # noqa: E731
    ops.launch("nrhip_packed_distortion_loss", live(s), live(e), live(w), seg, R, M, loss, grad if want_grad else None)
    return loss, grad


def launch_carving(ops, d, R, M, did_return=True, weights=True, mask=True):
    close = torch.full((M + SPARE,), 255, dtype=torch.uint8, device="cuda")
    loss, grad = nan_rows(R), nan_rows(M)
    live = lambda t: t if M else None  # noqa: E731
    ops.launch("nrhip_packed_lidar_carving", live(d["t_starts"]), live(d["t_ends"]), live(d["weights"]) if weights else None,
               d["seg"], d["is_lidar"], d["did_return"] if did_return else None, d["distance"], P.EPS, P.NON_RETURN, R, M,
               close if mask else None, loss if weights else None, grad if weights else None)
    return close, loss, grad


# ---- the distortion loss -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [R_FULL, R_PART], ids=["full-blocks", "partial-last-block"])
def test_distortion_value_and_gradient_against_the_float64_quadratic_form(ops, dist, R):
    s, e, w, seg = dist["dev"]
    M = int(dist["host"][3][R])
    loss, grad = launch_distortion(ops, s, e, w, seg, R, M)
    torch.cuda.synchronize()
    lo, gr = host64(loss), host64(grad)
    err_l, err_g = np.abs(lo[:R] - dist["loss"][:R]), np.abs(gr[:M] - dist["grad"][:M])
    print("worst loss error / bound", float(np.max(err_l / np.maximum(dist["loss_bound"][:R], 1e-300))),
          " worst gradient error / bound", float(np.max(err_g / np.maximum(dist["grad_bound"][:M], 1e-300))))
    assert np.all(err_l <= dist["loss_bound"][:R]), np.flatnonzero(err_l > dist["loss_bound"][:R])
    assert np.all(err_g <= dist["grad_bound"][:M]), np.flatnonzero(err_g > dist["grad_bound"][:M])
    # every live row written, none behind them; an empty ray writes 0
    assert np.all(np.isnan(lo[R:])) and np.all(np.isnan(gr[M:]))
    empty = dist["n"][:R] == 0
    assert empty.sum() >= 4 and np.all(lo[:R][empty] == 0) and not np.any(np.signbit(lo[:R][empty]))
    assert np.all(lo[:R] >= 0) and (dist["loss"][:R] > 1e-3).sum() >= 12 and np.all(lo[:R][dist["loss"][:R] > 1e-30] > 0)
    # the same launch again: the same bits; without grad_w (one walk): the same loss
    loss2, grad2 = launch_distortion(ops, s, e, w, seg, R, M)
    loss3, grad3 = launch_distortion(ops, s, e, w, seg, R, M, want_grad=False)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(grad2), bits(grad))
    assert torch.equal(bits(loss3), bits(loss)) and bool(torch.isnan(grad3).all())


def test_distortion_without_samples_zeroes_the_rays_and_reads_no_sample(ops):
    R = 7
    loss, grad = launch_distortion(ops, None, None, None, torch.zeros(R + 1, dtype=torch.int64, device="cuda"), R, 0)
    torch.cuda.synchronize()
    assert bool((loss[:R] == 0).all()) and bool(torch.isnan(loss[R:]).all()) and bool(torch.isnan(grad).all())
    out, g = ops.packed_distortion_loss_rays(*(torch.zeros(0, device="cuda"),) * 3,
                                             torch.zeros(R + 1, dtype=torch.int64, device="cuda"))
    assert out.shape == (R,) and bool((out == 0).all()) and g.shape == (0,)


# ---- lidar carving -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [R_FULL, R_PART], ids=["full-blocks", "partial-last-block"])
def test_carving_mask_loss_and_gradient(ops, carve, R):
    c, d = carve["host"], carve["dev"]
    M = int(c["seg"][R])
    close, loss, grad = launch_carving(ops, d, R, M)
    torch.cuda.synchronize()
    mask = host(close)
    assert np.array_equal(mask[:M], carve["mask"][:M].view(np.uint8)), "the mask is the reference's, bit for bit"
    assert np.all(mask[M:] == 255)
    lo, n = host64(loss), np.diff(c["seg"])[:R].astype(np.float64)
    err = np.abs(lo[:R] - carve["loss"][:R])
    bound = P.carving_loss_bound(carve["loss"][:R], n, carve["loss"][:R])
    print("worst carving loss error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound) and np.all(np.isnan(lo[R:]))
    assert np.array_equal(host(grad)[:M].view(np.int32), carve["grad"][:M].view(np.int32)), "2 wf is exact in fp32"
    assert np.all(np.isnan(host(grad)[M:]))
    # empty rays write 0; a camera ray contributes 0 and gets zero gradient whatever its samples hold
    assert np.all(lo[:R][n == 0] == 0)
    cam = ~c["is_lidar"][:R]
    rep = np.repeat(cam, np.diff(c["seg"])[:R])
    assert (cam & (n > 0)).sum() >= 4 and np.all(lo[:R][cam] == 0) and np.all(host(grad)[:M][rep] == 0)
    assert not mask[:M][rep].any() and np.abs(c["weights"][:M][rep]).max() > 0.5
    assert lo[:R].max() > 0.1 and (carve["grad"][:M] != 0).sum() > 100
    # the same launch again: the same bits; the mask alone (no weights): the same mask
    close2, loss2, grad2 = launch_carving(ops, d, R, M)
    close3, _, _ = launch_carving(ops, d, R, M, weights=False)
    assert torch.equal(close2, close) and torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(grad2), bits(grad))
    assert torch.equal(close3, close)


def test_carving_without_did_return_is_all_returned(ops, carve):
    c, d = carve["host"], carve["dev"]
    M = int(c["seg"][R_FULL])
    null = launch_carving(ops, d, R_FULL, M, did_return=False)
    ones = launch_carving(ops, {**d, "did_return": torch.ones_like(d["did_return"])}, R_FULL, M)
    for a, b in zip(null, ones):
        assert torch.equal(bits(a), bits(b))
    assert np.array_equal(host(null[0])[:M], carve["mask_all_returned"].view(np.uint8))
    assert not np.array_equal(carve["mask_all_returned"], carve["mask"])


def test_carving_without_samples_zeroes_the_rays(ops, carve):
    R = 6
    d = {**carve["dev"], "seg": torch.zeros(R + 1, dtype=torch.int64, device="cuda")}
    close, loss, grad = launch_carving(ops, d, R, 0)
    torch.cuda.synchronize()
    assert bool((loss[:R] == 0).all()) and bool(torch.isnan(loss[R:]).all()) and bool(torch.isnan(grad).all())
    assert bool((close == 255).all())
    z = torch.zeros(0, device="cuda")
    mask, out, g = ops.packed_lidar_carving(z, z, d["seg"], d["is_lidar"][:R].bool(), None, d["distance"][:R], P.EPS,
                                            P.NON_RETURN, weights=z)
    assert mask.shape == (0,) and g.shape == (0,) and out.shape == (R,) and bool((out == 0).all())


# ---- the public functions ------------------------------------------------------------------------------------------------
def test_public_functions_addressings_shapes_and_autocast(ops, dist, carve):
    from neurad_studio_amd.model_components.lidar_losses import packed_carving_loss, packed_is_close_to_lidar
    from neurad_studio_amd.model_components.losses import packed_distortion_loss

    s, e, w, seg = dist["dev"]
    R = R_FULL
    ri = ops.packed_ray_indices(seg, w.shape[0])
    c = carve["dev"]
    lid, ret = c["is_lidar"].bool(), c["did_return"].bool()
    carve_args = (lid, ret, c["distance"], P.EPS, P.NON_RETURN)

    def both(weights, **where):
        """-> (distortion, its gradient, carving, its gradient) for one way of passing the weights and the addressing"""
        out = []
        for fn in (lambda x: packed_distortion_loss(x, s, e, **where),
                   lambda x: packed_carving_loss(x, c["t_starts"], c["t_ends"], *carve_args, **where)):
            x = weights.clone().requires_grad_(True)
            v = fn(x)
            assert v.shape == () and v.dtype == torch.float32
            v.backward()
            assert x.grad.shape == x.shape
            out += [v.detach(), x.grad.reshape(-1)]
        return out

    base = both(w, segments=seg)
    for other in (both(w, ray_indices=ri, num_rays=R), both(w[:, None], segments=seg),
                  both(w[:, None], ray_indices=ri, num_rays=R)):
        for a, b in zip(base, other):
            assert torch.equal(bits(a), bits(b))
    # analytic: the mean over ALL rays of the kernel's per-ray values, the saved gradient times go / R; the sum over the rays
    per_ray, g = ops.packed_distortion_loss_rays(s, e, w, seg)
    assert torch.equal(base[0], per_ray.sum() / R) and torch.equal(base[1], g * (torch.ones((), device="cuda") / R))
    _, cl, cg = ops.packed_lidar_carving(c["t_starts"], c["t_ends"], seg, lid, ret, c["distance"], P.EPS, P.NON_RETURN,
                                         weights=c["weights"], want_mask=False)
    x = c["weights"].clone().requires_grad_(True)
    v = packed_carving_loss(x, c["t_starts"], c["t_ends"], *carve_args, segments=seg)
    (3.0 * v).backward()
    assert torch.equal(v.detach(), cl.sum()) and torch.equal(x.grad, cg * 3.0)
    # fp16 weights under autocast: the fp32 result on the same (fp16-representable) weights
    wh = w.half()
    exact = both(wh.float(), segments=seg)
    with torch.autocast("cuda", dtype=torch.float16):
        cast = both(wh, segments=seg)
    for k in (0, 2):  # the values: fp32, the same bits
        assert cast[k].dtype == torch.float32 and torch.equal(bits(exact[k]), bits(cast[k]))
    for k in (1, 3):  # the gradients come back through the cast: the fp32 ones rounded to the weights' fp16
        assert cast[k].dtype == torch.float16 and torch.equal(exact[k].half(), cast[k])
    # the mask, with distance given as [R,1]
    close = packed_is_close_to_lidar(c["t_starts"][:, None], c["t_ends"][:, None], lid, ret, c["distance"][:, None], P.EPS,
                                     P.NON_RETURN, ray_indices=ri, num_rays=R)
    assert close.dtype == torch.bool and close.shape == (w.shape[0],) and np.array_equal(host(close), carve["mask"])


# ---- through the fused packed training node ---------------------------------------------------------------------------------
def test_losses_on_the_fused_packed_training_node(ops):
    """features.sum() + a carving + b distortion on render_train_packed's outputs: the loss values are the kernels' on the
    node's weights, weights.grad is a grad_carving + b grad_distortion, and the table's gradient feels the two terms"""
    from neurad_studio_amd.model_components.lidar_losses import packed_carving_loss
    from neurad_studio_amd.model_components.losses import packed_distortion_loss

    fld, _ = T.make_field(4, 2, 32, True)
    rays = T.packed_rays(T.RAGGED, 7)
    o, d, area, ts, te, seg, ri = T.on_device(rays)
    R, counts = len(T.RAGGED), np.asarray(T.RAGGED)
    rng = np.random.default_rng(8)
    is_lidar = np.arange(R) % 2 == 0
    did_return = np.arange(R) % 4 == 0
    distance = rng.uniform(10.0, 50.0, R).astype(np.float32)
    eps, non_return = 4.0, 30.0
    lid, ret, dist_d = cuda(is_lidar), cuda(did_return), cuda(distance)
    table = fld.hashgrid.static_grid.hash_table

    def step(a, b):
        fld.zero_grad()
        f, _, _, w = fld.render_train_packed(o, d, area, ts, te, segments=seg)
        w.retain_grad()
        lc = packed_carving_loss(w, ts, te, lid, ret, dist_d, eps, non_return, segments=seg)
        ld = packed_distortion_loss(w, ts, te, segments=seg)
        (f.sum() + a * lc + b * ld).backward()
        return w.detach(), lc.detach(), ld.detach(), (None if w.grad is None else w.grad.clone()), table.grad.clone()

    a, b = 0.5, 2.0
    w, lc, ld, gw, gt = step(a, b)
    _, kl, kg = ops.packed_lidar_carving(ts, te, seg, lid, ret, dist_d, eps, non_return, weights=w, want_mask=False)
    per_ray, _ = ops.packed_distortion_loss_rays(ts, te, w, seg)
    assert torch.equal(lc, kl.sum()) and torch.equal(ld, per_ray.sum() / R)
    # weights.grad against the float64 references on the node's own weights: the kernels' bounds, scaled by a and b / R, plus
    # the fp32 roundings of putting the two together (b / R, its product with the gradient, the sum: 2^-24 each on terms of
    # at most |a g_c| + |b / R g_d|)
    wh, tsh, teh, segh = host(w), rays[3], rays[4], rays[5]
    mask = P.carving_mask(tsh, teh, segh, is_lidar, did_return, distance, eps, non_return)
    _, gc = P.carving_loss(wh, mask, segh, is_lidar)
    _, gd = P.distortion_quadratic(tsh, teh, wh, segh)
    n, X, S = P.distortion_scales(tsh, teh, wh, segh)
    want = a * gc.astype(np.float64) + (b / R) * gd
    tol = (b / R) * P.grad_bound(gd, n, X, S, segh) + 4 * P.U32 * (np.abs(a * gc) + np.abs((b / R) * gd))
    err = np.abs(host64(gw) - want)
    print("worst weights.grad error / bound", float(np.max(err / np.maximum(tol, 1e-300))))
    assert np.all(err <= tol), np.flatnonzero(err > tol)
    assert (mask & np.repeat(is_lidar, counts)).sum() > 20 and (gc != 0).sum() > 0 and float(lc) > 0 and float(ld) > 0
    # the table's gradient is finite and is not the one of features.sum() alone
    _, _, _, _, gt0 = step(0.0, 0.0)
    assert bool(torch.isfinite(gt).all()) and bool(torch.isfinite(gt0).all())
    assert not torch.equal(gt, gt0) and float((gt.float() - gt0.float()).abs().max()) > 0


def test_lidar_metrics_without_proposal_rounds_on_the_occupancy_route(ops):
    """lidar_metrics(..., num_proposal_rounds=0) on VolumetricSampler.render_train's outputs with the packed carving term:
    runs, backpropagates, and its carving_loss is packed_carving_loss / n_lidar"""
    from neurad_studio_amd.model_components.lidar_losses import LidarLossSettings, lidar_metrics, packed_carving_loss
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    R = 96
    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    est.binaries[0] = cuda(np.random.default_rng(3).random((16, 16, 16)) < 0.3)
    sampler = VolumetricSampler(est).train()
    fld, _ = T.make_field(4, 2, 32, True)
    rb = ray_bundle(R, 90, far=9.0)
    out = sampler.render_train(fld, rb, render_step_size=0.1, cone_angle=0.0)
    M = out["ray_indices"].shape[0]
    assert M > 1000 and out["weights"].shape == (M, 1)
    torch.manual_seed(4)
    is_lidar = torch.arange(R, device="cuda") % 2 == 0
    n_lidar = R // 2
    did_return = torch.rand(n_lidar, device="cuda") < 0.7
    distance = torch.rand(n_lidar, 1, device="cuda") * 7 + 1
    cfg = LidarLossSettings(non_return_lidar_distance=6.0)
    ret_all = torch.ones(R, dtype=torch.bool, device="cuda")
    dist_all = torch.zeros(R, device="cuda")
    ret_all[is_lidar], dist_all[is_lidar] = did_return, distance[:, 0]  # per RAY of the batch: what the packed term takes
    carving = packed_carving_loss(out["weights"], out["t_starts"], out["t_ends"], is_lidar, ret_all, dist_all, 0.5,
                                  cfg.non_return_lidar_distance, ray_indices=out["ray_indices"], num_rays=R)
    intensity = torch.rand(n_lidar, 1, device="cuda").requires_grad_(True)
    logits = torch.randn(n_lidar, 1, device="cuda").requires_grad_(True)
    outputs = {"depth": out["depth"], "intensity": intensity, "ray_drop_logits": logits, "non_nearby_weights_loss": carving}
    m = lidar_metrics(outputs, is_lidar, did_return, distance, torch.rand(n_lidar, 1, device="cuda"), cfg,
                      num_proposal_rounds=0)
    assert set(m) == {"depth_loss", "intensity_loss", "ray_drop_loss", "carving_loss"}
    assert float(carving.detach()) > 0 and torch.equal(m["carving_loss"], carving / n_lidar)
    sum(m.values()).backward()
    gt = fld.hashgrid.static_grid.hash_table.grad
    assert all(bool(torch.isfinite(v).all()) for v in m.values())
    assert gt is not None and bool(torch.isfinite(gt).all()) and float(gt.float().abs().max()) > 0
    assert intensity.grad is not None and logits.grad is not None
