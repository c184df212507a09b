"""The kernels of the VGG perceptual loss (csrc/vgg_loss.hip) one by one, exact where they can be.

conv3x3: integer operands (tests/vgg_refs.py derives why every product, every fp32 partial sum and the fp16 result are then
exact, and asserts the operands qualify), so the kernel must return the float64 reference bit for bit -- forward with bias
and ReLU, and the input gradient with the ReLU mask, for all 16 channel pairs, in both launch-plan branches.  The plan has
one branch point, the 32-pixel blocks per wave (1 or 2; the 32-channel blocks follow from the output width alone), and the
pixel tiling runs over the flattened batch, so the shapes are counted in pixels of a tile T = 32 * blocks:
  (1,1,1) one pixel; (1,1,T-1) and (1,T-1,1) one ragged tile as a row and as a column; (1,1,T+1) and (1,T+1,1) two tiles with
  a single pixel in the second; (3,6,6) 108 pixels whose tiles cross the image boundaries; (2,5,7) two images of an odd size.
Which branch a case reaches is asserted from nrhip_conv3x3_plan next to it: these shapes choose 1 block on their own, 2
blocks are forced there, and one case (3 -> 64 at 2 x 256 x 256) reaches 2 blocks through the plan's own choice.
Output buffers are NaN-prefilled: an unwritten element shows.

maxpool and the L1 backward are exact too; the L1 forward is held to 8 u |ref| (float64 partials, one rounding: a bound
with room, not a measured one)."""
import math

import pytest
import torch

import vgg_refs as R

pytestmark = pytest.mark.gpu

PAIRS = [(a, b, m) for a, b in R.CHANNEL_PAIRS for m in (0, 1)]


def _V():
    from neurad_studio_amd import ops_vgg

    return ops_vgg


def _nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float16)


def _run_conv_case(V, c, cin, cout, mode, blocks, what):
    b, h, w = c["x" if mode == 0 else "g"].shape[:3]
    m = b * h * w
    if mode == 0:
        mt, nt, waves = V.conv3x3_plan(m, cin, cout, blocks)
        assert (mt, nt) == (blocks or mt, 2) and waves == -(-m // (32 * mt)) * (cout // 64)
        out = V.conv3x3(c["x"].cuda(), V.conv3x3_pack(c["w"].cuda(), 0), cin, cout, bias=c["bias"].cuda(), relu=True,
                        plan=blocks, out=_nan_like(c["out"].shape))
        R.assert_equal(out, c["out"], f"{what} forward")
    else:  # the input gradient: the same kernel on the mode-1 pack, channels swapped
        mt, nt, waves = V.conv3x3_plan(m, cout, cin, blocks)
        assert (mt, nt) == (blocks or mt, 1 if cin == 3 else 2) and waves == -(-m // (32 * mt)) * max(cin // 64, 1)
        gx = V.conv3x3(c["g"].cuda(), V.conv3x3_pack(c["w"].cuda(), 1), cout, cin, mask=None if cin == 3 else c["act"].cuda(),
                       plan=blocks, out=_nan_like(c["gx"].shape))
        R.assert_equal(gx, c["gx"], f"{what} input gradient")
    return mt


@pytest.mark.parametrize("cin,cout,mode", PAIRS, ids=[f"{a}to{b}-{'bwd' if m else 'fwd'}" for a, b, m in PAIRS])
def test_conv3x3_is_exact_in_both_pack_modes_and_plan_branches(cin, cout, mode):
    V = _V()
    for blocks in (1, 2):
        for k, (b, h, w) in enumerate(R.conv_shapes(blocks)):
            c = R.conv_case(b, h, w, cin, cout, seed=1000 * blocks + 10 * k + mode, mode=mode)
            # these sizes choose one block on their own (asserted); two blocks are forced
            assert V.conv3x3_plan(b * h * w, *((cin, cout) if mode == 0 else (cout, cin)))[0] == 1
            mt = _run_conv_case(V, c, cin, cout, mode, 0 if blocks == 1 else 2, f"conv3x3 {cin}->{cout} blocks={blocks} {(b, h, w)}")
            assert mt == blocks


def test_conv3x3_reaches_two_blocks_by_its_own_plan():
    """2 x 256 x 256 pixels at 64 output channels: 2048 waves of 64 pixels, the threshold itself; one pixel fewer per image
    row keeps one block"""
    V = _V()
    assert V.conv3x3_plan(2 * 256 * 256, 3, 64) == (2, 2, 2048) and V.conv3x3_plan(2 * 256 * 255, 3, 64)[0] == 1
    c = R.conv_case(2, 256, 256, 3, 64, seed=7, mode=0)
    assert _run_conv_case(V, c, 3, 64, 0, 0, "conv3x3 3->64 auto plan 2x256x256") == 2


def test_conv3x3_refuses_what_it_does_not_support():
    V = _V()
    x = torch.zeros((1, 4, 4, 64), device="cuda", dtype=torch.float16)
    wf = V.conv3x3_pack(torch.zeros((64, 64, 3, 3), device="cuda"), 0)
    with pytest.raises(ValueError):
        V.conv3x3(x, wf, 64, 128)  # a pack of another shape
    with pytest.raises(ValueError):
        V.conv3x3(x[..., :32].contiguous(), wf, 32, 64)
    with pytest.raises(ValueError):
        V.conv3x3(x, wf, 64, 64, mask=x[:, :2])


# ---- maxpool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (1, 17, 19, 64), (3, 2, 2, 8), (1, 3, 5, 128)], ids=str)
def test_maxpool_forward_and_backward_are_exact_with_torchs_ties(shape):
    """values from {0, 0, 1, 2, 3} / 4: ties in most windows, all-zero windows, ties among positive values; a first channel
    all equal; the gradient goes to the first maximum in row-major order, the dropped row and column get exactly zero"""
    V = _V()
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randint(0, 5, shape, generator=g).clamp_min(1) - 1).half() / 4
    x[..., 0] = 0.75  # every window of this channel is all-equal
    ref = R.pool_fwd(x)
    out = V.maxpool2_fwd(x.cuda())
    R.assert_equal(out, ref.half(), f"maxpool2_fwd {shape}")
    go = torch.randint(-8, 9, ref.shape, generator=g).half() / 8
    states = V.new_states(2, "cuda")
    states[0] = torch.tensor([float(go.abs().max()), 4.0])
    p = R.pow2_norm(float(go.abs().max()))
    gin = V.maxpool2_bwd(x.cuda(), go.cuda(), in_state=states[0], out_state=states[1])
    want = R.pool_bwd(x, go.double() * p)
    R.assert_equal(gin, want.half(), f"maxpool2_bwd {shape}")
    assert states[1].tolist() == [float(go.abs().max()) * p, 4.0 * p]
    h, w = shape[1], shape[2]
    if h % 2:
        assert not gin[:, h - 1].any()
    if w % 2:
        assert not gin[:, :, w - 1].any()
    win = R.pool_windows(gin.cpu().double())
    assert int((win != 0).sum(-1).max()) <= 1  # one position per window at most
    assert torch.equal(win[..., 0, :].sum(-1), go[..., 0].double() * p)  # all-equal windows: the first position takes it
    assert not win[..., 0, 1:].any()


# ---- L1 -------------------------------------------------------------------------------------------------------------------
L1_SIZES = [1, 7, 2047, 2048, 2049, 5 * 2048 + 3]


def _l1_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    fx = (torch.rand(n, generator=g) * 4).half()
    fy = (torch.rand(n, generator=g) * 4).half()
    fy[2::3] = fx[2::3]  # equal features: a zero gradient
    fx[1::5] = 0         # ReLU zeros
    return fx, fy


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_forward_against_float64_and_run_to_run(n):
    """one element, one workgroup - 1 / exactly / + 1, several workgroups; aligned (16-byte loads) and misaligned views"""
    from neurad_studio_amd._lib import L1_ITEMS

    assert L1_ITEMS == 2048
    V = _V()
    fx, fy = _l1_inputs(n, n)
    ref = float((fx.double() - fy.double()).abs().mean())
    base = torch.zeros(n + 8, device="cuda", dtype=torch.float16)
    for off in (0, 1):  # offset 1: a 2-byte aligned view, the element-wise path
        a, b = base[off:off + n].copy_(fx), fy.cuda()
        got = V.l1_feature_fwd(a, b)
        err = abs(float(got) - ref)
        print(f"[vgg-kernels] l1 fwd n={n} off={off}: err / (u |ref|) = {err / (R.U32 * ref):.3g}")
        assert err <= 8 * R.U32 * ref
        again = V.l1_feature_fwd(a, b)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        acc = V.l1_feature_fwd(a, b, weight=0.25, accum=got)
        assert abs(float(acc) - 1.25 * ref) <= 8 * R.U32 * 1.25 * ref


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_backward_is_one_fp16_rounding_and_zero_where_equal(n):
    V = _V()
    fx, fy = _l1_inputs(n, 100 + n)
    w, g = 0.125, torch.tensor([0.37], device="cuda")
    states = V.new_states(2, "cuda")
    got = V.l1_feature_bwd(fx.cuda(), fy.cuda(), w, g, states[0])
    amax, s = states[0].tolist()
    c = float(torch.tensor(w, dtype=torch.float32).double() * g.cpu().double() / n)
    assert s == R.pow2_norm(abs(c)) and 0.5 <= amax < 1 and amax == float(got.abs().max())
    true = got.cpu().double() / s
    ref = c * torch.sign(fx.double() - fy.double())
    assert float(((true - ref).abs() - R.U16 * ref.abs()).max()) <= 0
    assert not true[fx == fy].any() and true[fx != fy].all()
    masked = V.l1_feature_bwd(fx.cuda(), fy.cuda(), w, g, states[1], mask_fx=True)
    assert torch.equal(masked.cpu(), torch.where(fx > 0, got.cpu(), torch.zeros((), dtype=torch.float16)))
    again = V.l1_feature_bwd(fx.cuda(), fy.cuda(), w, g, V.new_states(1, "cuda")[0])
    assert torch.equal(got, again)


# ---- working scale --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2.0 ** 16, 2.0 ** -16], ids=["x2^16", "x2^-16"])
def test_working_scale_carries_a_power_of_two_exactly(k):
    """tap gradient -> convolution input gradient (mask) -> pool backward -> merge with a second tap -> convolution to the image:
    with the incoming gradient multiplied by 2^16 or 2^-16 every stored fp16 tensor keeps its bits and the fp32 result is the
    unscaled one times that power of two, bit for bit"""
    V = _V()
    gen = torch.Generator().manual_seed(11)
    b, h, w = 2, 6, 10
    f2 = torch.rand((2 * b, h // 2, w // 2, 128), generator=gen).half().cuda()   # the deeper tap's features
    f1 = (torch.rand((2 * b, h, w, 64), generator=gen) - 0.3).clamp_min(0).half().cuda()  # pool input, and the shallower tap
    act = (torch.rand((b, h // 2, w // 2, 64), generator=gen) - 0.3).half().cuda()
    w2 = (torch.randn((128, 64, 3, 3), generator=gen) * 0.05).cuda()
    w1 = (torch.randn((64, 3, 3, 3), generator=gen) * 0.2).cuda()
    p2, p1 = V.conv3x3_pack(w2, 1), V.conv3x3_pack(w1, 1)

    def chain(g):
        st = V.new_states(5, "cuda")
        g2 = V.l1_feature_bwd(f2[:b], f2[b:], 1.0, g, st[0], mask_fx=True)
        ga = V.conv3x3(g2, p2, 128, 64, mask=act, in_state=st[0], out_state=st[1])
        gp = V.maxpool2_bwd(f1[:b], ga, in_state=st[1], out_state=st[2])
        gm = V.l1_feature_bwd(f1[:b], f1[b:], 0.03125, g, st[3], mask_fx=True, above=gp, above_state=st[2])
        gi = V.conv3x3(gm, p1, 64, 3, in_state=st[3], out_state=st[4])
        return V.image_grad(gi, st[4]), (g2, ga, gp, gm, gi), st

    g = torch.tensor([0.8125], device="cuda")
    base, stored, st = chain(g)
    scaled, stored_k, st_k = chain(g * k)
    assert float(base.abs().max()) > 0 and torch.isfinite(base).all()
    for a, c in zip(stored, stored_k):
        assert torch.equal(a, c)
    assert torch.equal(st[:, 0], st_k[:, 0]) and torch.equal(st[:, 1], st_k[:, 1] * k)
    assert torch.equal(scaled, base * k)
    for s in st[:, 1].tolist():
        assert math.frexp(s)[0] == 0.5  # every scale is a power of two
    amax = [float(t.abs().max()) for t in stored]
    assert st[:, 0].tolist() == amax  # the tracked maxima are the tensors' own
    # a non-finite incoming gradient poisons the result, as it would under AMP
    poisoned, _, _ = chain(g * float("inf"))
    assert torch.isnan(poisoned).all()


def test_stage_and_image_grad():
    V = _V()
    x, y = R.make_images(2, 5, 7)
    img = V.stage_images(x.cuda(), y.cuda())
    assert img.shape == (4, 5, 7, 16) and not img[..., 3:].any()
    assert torch.equal(img[..., :3].cpu(), torch.cat([x, y]).half())
    g16 = torch.randn((2, 5, 7, 16), generator=torch.Generator().manual_seed(2)).half()
    st = torch.tensor([1.0, 2.0 ** 20], device="cuda")
    assert torch.equal(V.image_grad(g16.cuda(), st).cpu(), g16[..., :3].float() * 2.0 ** -20)
