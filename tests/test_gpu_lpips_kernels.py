"""The kernels of LPIPS (csrc/lpips.hip) one by one, exact where they can be.

conv2d: integer operands (tests/lpips_refs.py and vgg_refs.py derive why every product, every fp32 partial sum and the fp16
result are then exact, and assert the operands qualify), so the kernel must return the float64 convolution + bias + ReLU
rounded to fp16 bit for bit, for each of AlexNet's five layers in both branches of the plan (1 or 2 32-pixel blocks per
wave; the plan has no other branch point).  Sizes: for the image layer 35 x 47 and 31 x 31 (8 x 11 and 7 x 7 outputs) and
33 x 38, where the last stride-4 window stops short of the edge (lpips_refs.conv_case_sizes says why the first two do not),
for the others 8 x 11 and 1 x 1 maps, each with B = 1 and B = 3, so tiles of 32 and 64 pixels cross rows and images and end
ragged.  One case per layer has a non-zero value in every border pixel; every case has negative pre-activations
(asserted in the builder).  Output buffers are NaN-prefilled: an unwritten element shows.  No layer uses the fp16-pair form
(DESIGN.md §8 has the emulation that decided it), so there is no inexact convolution case.

The pool and the staging are exact as well; the head is held to the bound tests/lpips_refs.py derives from fp32 round-off
over C channels."""
import pytest
import torch

import lpips_refs as R

pytestmark = pytest.mark.gpu


def _L():
    from neurad_studio_amd import ops_lpips

    return ops_lpips


def _nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float16)


@pytest.mark.parametrize("layer", range(5), ids=[f"{s[0]}to{s[1]}k{s[2]}" for s in R.CONV_SHAPES])
def test_conv2d_is_exact_in_both_plan_branches(layer):
    L = _L()
    shape = R.CONV_SHAPES[layer]
    cin, cout, ks, stride, pad = shape
    for k, (b, h, w) in enumerate(R.conv_case_sizes(layer)):
        c = R.conv_case(b, h, w, layer, seed=100 * layer + k, border=(k == 1))
        wf = L.conv2d_pack(c["w"].cuda())
        m = b * R.out_size(h, ks, stride, pad) * R.out_size(w, ks, stride, pad)
        assert tuple(c["out"].shape) == (b, R.out_size(h, ks, stride, pad), R.out_size(w, ks, stride, pad), cout)
        for blocks in (0, 1, 2):
            mt, nt, waves = L.conv2d_plan(m, shape, blocks)
            assert (mt, nt) == (blocks or 1, 2) and waves == -(-m // (32 * mt)) * (cout // 64)
            out = L.conv2d(c["x"].cuda(), wf, shape, bias=c["bias"].cuda(), relu=True, plan=blocks, out=_nan_like(c["out"].shape))
            R.assert_equal(out, c["out"], f"layer {layer} {b}x{h}x{w} plan {blocks}")


def test_conv2d_without_bias_and_relu_keeps_negative_sums():
    L = _L()
    c = R.conv_case(1, 8, 11, 2, seed=7)
    cin, cout, ks, stride, pad = R.CONV_SHAPES[2]
    want = torch.nn.functional.conv2d(R.nchw(c["x"].double()), c["w"].double(), padding=pad)
    assert float(want.min()) < 0
    out = L.conv2d(c["x"].cuda(), L.conv2d_pack(c["w"].cuda()), R.CONV_SHAPES[2], relu=False)
    R.assert_equal(out, R.nhwc(want).half(), "no bias, no ReLU")


def test_the_plan_chooses_two_blocks_on_its_own_for_a_large_map():
    """2 x 134 x 239 pool-1 outputs (a 1080 x 1920 pair) reach mt = 2 through the plan's own choice: the same bits as mt = 1"""
    L = _L()
    shape = R.CONV_SHAPES[1]
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(-2, 3, (2, 134, 239, 64), generator=g) * (torch.rand((2, 134, 239, 64), generator=g) < 0.25)).half().cuda()
    c = R.conv_case(1, 1, 1, 1, seed=11)
    assert L.conv2d_plan(2 * 134 * 239, shape, 0)[0] == 2
    R.assert_exact_operands(torch.nn.functional.conv2d(R.nchw(x[:1, 60:67].double().cpu()).abs(), c["w"].double().abs(),
                                                       c["bias"].double().abs(), padding=2))
    wf, bias = L.conv2d_pack(c["w"].cuda()), c["bias"].cuda()
    a, b = L.conv2d(x, wf, shape, bias=bias, plan=0), L.conv2d(x, wf, shape, bias=bias, plan=1)
    assert torch.equal(a, b) and float(a.float().abs().max()) > 0
    # one row of it against float64 (integers: exact)
    want = torch.nn.functional.conv2d(R.nchw(x[:1, 60:67].double().cpu()), c["w"].double(), c["bias"].double(), padding=2)
    R.assert_equal(a[:1, 62:65], R.nhwc(want.clamp_min(0))[:, 2:5].half(), "rows 62..64 of the large map")


@pytest.mark.parametrize("b,h,w,c", [(1, 3, 3, 64), (1, 4, 4, 64), (2, 7, 8, 192), (3, 8, 11, 64), (1, 15, 6, 8)])
def test_maxpool3s2_equals_torch(b, h, w, c):
    L = _L()
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((b, h, w, c), generator=g).half()
    want = R.pool_ref(x)
    assert tuple(want.shape) == (b, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c)
    R.assert_equal(L.maxpool3s2_fwd(x.cuda()), want, f"pool {h}x{w}")


def _stage(L, a, b):
    shift, scale = torch.tensor(R.SHIFT).cuda(), torch.tensor(R.SCALE).cuda()
    return L.stage_images(R.nhwc(a).cuda(), R.nhwc(b).cuda(), shift, scale)


def test_staging_is_exact_and_the_flag_is_clear_in_range():
    L = _L()
    a, b = R.make_pair(2, 33, 37, "noise", seed=5)
    a[0, :, 0, 0], a[1, :, -1, -1] = 0.0, 1.0  # the ends of the range are inside it
    out, flag = _stage(L, a, b)
    want = R.nhwc(R.stage_ref(torch.cat([a, b]))).float().half()  # float64 -> fp32 -> fp16: torch's own double -> half path
    assert tuple(out.shape) == (4, 33, 37, R.IMAGE_CHANNELS)
    R.assert_equal(out[..., :3], want, "staged image")
    assert not bool(out[..., 3].any()) and int(flag) == 0


@pytest.mark.parametrize("bad", [-1e-3, 1 + 1e-3, float("nan"), float("inf")], ids=["below", "above", "nan", "inf"])
@pytest.mark.parametrize("second", [False, True], ids=["first", "second"])
def test_staging_flags_a_value_out_of_range_at_the_last_pixel(bad, second):
    L = _L()
    a, b = R.make_pair(1, 31, 33, "noise", seed=6)
    (b if second else a)[0, 2, -1, -1] = bad
    assert int(_stage(L, a, b)[1]) == 1


HEAD_CASES = [(c, p, b) for c in (64, 192, 384, 256) for p, b in ((1, 1), (31, 2), (32, 1), (33, 2), (63, 2), (64, 1), (65, 2), (9 * 32 + 5, 2))]


@pytest.mark.parametrize("c,pixels,b", HEAD_CASES, ids=[f"c{c}-p{p}-b{b}" for c, p, b in HEAD_CASES])
def test_head_meets_its_bound_in_both_eps_placements(c, pixels, b):
    L = _L()
    f, lin = R.head_case(b, pixels, c, seed=c + pixels)
    feat = f.reshape(2 * b, 1, pixels, c).cuda()
    for mode in (R.EPS_INSIDE, R.EPS_OUTSIDE):
        want, bound = R.head_out_ref(f, lin, mode)
        got = L.lpips_head(feat, lin.cuda(), mode)
        err = (got.double().cpu() - want).abs()
        print(f"head c={c} pixels={pixels} mode={mode}: err {float(err.max()):.3e} bound {float(bound.min()):.3e}")
        assert bool((err <= bound).all()), (err, bound)
        assert float(want.min()) > 0.01  # the case says something
        again = L.lpips_head(feat, lin.cuda(), mode)
        assert torch.equal(got, again)  # the same bits on two consecutive runs
        # accumulation into an existing out
        acc = torch.full((b,), 0.375, device="cuda")
        L.lpips_head(feat, lin.cuda(), mode, out=acc)
        want2, bound2 = R.head_out_ref(f, lin, mode, accum=torch.full((b,), 0.375))
        assert bool(((acc.double().cpu() - want2).abs() <= bound2).all())


@pytest.mark.parametrize("mode", [R.EPS_INSIDE, R.EPS_OUTSIDE])
def test_head_zero_pixels(mode):
    """a pixel that is all zero in both images contributes exactly 0; zero in one image only it contributes sum_c lin_c n_c^2
    of the other"""
    L = _L()
    c = 64
    f = torch.zeros((2, 2, c), dtype=torch.float16)
    lin = torch.rand((c,), generator=torch.Generator().manual_seed(1))
    got = L.lpips_head(f.reshape(2, 1, 2, c).cuda(), lin.cuda(), mode)
    assert float(got) == 0.0  # all pixels zero in both: exactly 0, no NaN from 0 / 0
    f[0, 1] = torch.rand((c,), generator=torch.Generator().manual_seed(2)).half()
    want, bound = R.head_out_ref(f, lin, mode)
    got = L.lpips_head(f.reshape(2, 1, 2, c).cuda(), lin.cuda(), mode)
    assert float(want) > 0.1 and abs(float(got) - float(want)) <= float(bound)
    d, _ = R.head_pixels_ref(f, lin, mode)
    assert float(d[0, 0]) == 0.0
