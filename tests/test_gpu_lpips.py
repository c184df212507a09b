"""LPIPS end to end on the device (model_components/lpips.py on csrc/lpips.hip) against the float64 restatement of the metric
(tests/lpips_refs.py), with seeded weights under the documented state-dict keys (lin weights non-negative).

The condition is absolute: LPIPS is published to three decimals, so every case is within 5e-4 of float64.  Cases: 31 x 31 (the
smallest image the network takes), 35 x 47 and 67 x 131, B = 1 and B = 2, three contents -- independent noise (values near 0.9),
an image against itself (exactly 0) and an image against a copy perturbed by +-0.04 (values of 5.5e-3 .. 7e-3: the regime a
rendered image against its ground truth sits in).  Every case but the identical pair has a float64 value above 5e-3 (asserted;
the seeds were chosen on the CPU), otherwise the absolute bound would test nothing.  The CPU emulation of the kernels' number
formats stays below 8.5e-5 on these cases."""
import pytest
import torch

import lpips_refs as R

pytestmark = pytest.mark.gpu

CASES = [(h, w, b, c) for (h, w) in R.E2E_SIZES for b in (1, 2) for c in R.CONTENTS]


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(0)


@pytest.fixture(scope="module")
def metric(weights):
    from neurad_studio_amd.model_components.lpips import LPIPS

    m = LPIPS()
    m.load_state_dict(weights, strict=True)
    return m.cuda()


@pytest.mark.parametrize("h,w,b,content", CASES, ids=[f"{h}x{w}-b{b}-{c}" for h, w, b, c in CASES])
def test_lpips_is_within_5e_4_of_float64(metric, weights, h, w, b, content):
    x, y = R.make_pair(b, h, w, content)
    want = R.lpips_pairs_ref(x, y, weights)
    pairs, flag = metric.pairs(x.cuda(), y.cuda())
    got = metric(x.cuda(), y.cuda())
    print(f"{h}x{w} B={b} {content}: float64 {want.tolist()} device {pairs.tolist()}")
    assert got.shape == () and got.is_cuda and got.dtype == torch.float32 and int(flag) == 0
    if content == "same":
        assert float(want.abs().max()) == 0.0 and float(pairs.abs().max()) == 0.0 and float(got) == 0.0
    else:
        assert float(want.min()) > R.FLOOR
    assert float((pairs.double().cpu() - want).abs().max()) <= R.TOL
    assert abs(float(got) - float(want.mean())) <= R.TOL


def test_hwc_views_and_channels_last_give_the_same_bits(metric):
    x, y = R.make_pair(1, 35, 47, "near")
    x, y = x.cuda(), y.cuda()
    want = metric(x, y)
    assert torch.equal(metric(x[0].permute(1, 2, 0), y[0].permute(1, 2, 0)), want)
    assert torch.equal(metric(x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)), want)
    assert torch.equal(metric(x.double(), y.double()), want)  # non-fp32 inputs are cast


def test_both_eps_placements_reach_the_kernel(weights):
    from neurad_studio_amd.model_components.lpips import EPS_OUTSIDE, LPIPS

    m = LPIPS(eps_mode=EPS_OUTSIDE)
    m.load_state_dict(weights)
    m.cuda()
    x, y = R.make_pair(1, 35, 47, "noise")
    want = R.lpips_pairs_ref(x, y, weights, eps_mode=R.EPS_OUTSIDE)
    assert abs(float(m(x.cuda(), y.cuda())) - float(want)) <= R.TOL


def test_inputs_that_require_grad_and_small_images_are_refused(metric):
    x, y = R.make_pair(1, 31, 31, "near")
    with pytest.raises(NotImplementedError):
        metric(x.cuda().requires_grad_(), y.cuda())
    with pytest.raises(NotImplementedError):
        metric(x.cuda(), y.cuda().requires_grad_())
    with pytest.raises(ValueError, match="smaller than 31"):
        metric(x.cuda()[..., :30], y.cuda()[..., :30])


def test_weights_modified_in_place_are_picked_up(weights):
    from neurad_studio_amd.model_components.lpips import LPIPS

    m = LPIPS()
    m.load_state_dict(weights)
    m.cuda()
    x, y = R.make_pair(1, 35, 47, "noise")
    dx, dy = x.cuda(), y.cuda()
    first, packs = float(m(dx, dy)), m.packs()
    assert m.packs() is packs and float(m(dx, dy)) == first  # cached while nothing moves
    changed = {k: v.clone() for k, v in weights.items()}
    with torch.no_grad():
        conv = m.net.net.slice2[1]
        conv.weight.mul_(-0.5)
        changed["net.net.slice2.3.weight"] = conv.weight.cpu().clone()
        m.net.lin4.model[1].weight.mul_(3.0)
        changed["net.lin4.model.1.weight"] = m.net.lin4.model[1].weight.cpu().clone()
    second = float(m(dx, dy))
    assert m.packs() is not packs
    want = float(R.lpips_pairs_ref(x, y, changed))
    assert abs(second - want) <= R.TOL and abs(second - first) > 10 * R.TOL


def test_triple_is_the_three_calls_in_one_transfer(metric):
    from neurad_studio_amd import ops
    from neurad_studio_amd.model_components import image_metrics as IM

    x, y = R.make_pair(1, 35, 47, "near")
    da, db = x.cuda(), y.cuda()  # the reference's [1, C, H, W] views
    transfers = []

    def to_host(values):
        torch.cuda.set_sync_debug_mode("default")
        transfers.append(tuple(values.shape))
        return IM.scalars_to_host(values)

    metric.packs()  # (packing happens once per set of weights, not per image)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # nothing before the transfer synchronises
    try:
        got = IM.image_eval_metrics3(da, db, metric, to_host=to_host)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert transfers == [(4,)] and tuple(got) == IM.IMAGE_EVAL_KEYS3 and all(type(v) is float for v in got.values())
    psnr, ssim = ops.image_metrics(da, db)
    assert got == {"psnr": float(psnr), "ssim": float(ssim), "lpips": float(metric(da, db))}
    triple = IM.ImageEvalTriple(metric, to_host=to_host)
    assert (triple.lpips(da, db), triple.psnr(da, db), triple.ssim(da, db)) == (got["lpips"], got["psnr"], got["ssim"])
    assert transfers == [(4,)] * 2
    assert IM.lpips_eval_metric(da, db, metric, to_host=to_host) == got["lpips"] and transfers[-1] == (2,)
    # an out-of-range image: the ValueError torchmetrics raises, after the one read
    bad = da.clone()
    bad[0, 1, -1, -1] = 1.001
    n = len(transfers)
    with pytest.raises(ValueError, match=r"\[0,1\] range"):
        IM.image_eval_metrics3(bad, db, metric, to_host=to_host)
    with pytest.raises(ValueError, match=r"\[0,1\] range"):
        IM.ImageEvalTriple(metric, to_host=to_host).ssim(bad, db)
    with pytest.raises(ValueError, match=r"\[0,1\] range"):
        IM.lpips_eval_metric(db, bad, metric, to_host=to_host)
    assert len(transfers) == n + 3
