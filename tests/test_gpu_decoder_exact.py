"""The decoder's kernels (csrc/decoder.hip) element by element, at the smallest shape that reaches each launch-plan branch.
Integer operands make every layer but BatchNorm's normalisation and the sigmoid EXACT: the kernel must return the float64
reference bit for bit (tests/decoder_refs.py derives why and checks the operands).  The rest is held to per-element
bounds derived there, none measured.  Which plan branch a shape reaches is asserted from the library's own plan queries
(nrhip_conv7x7_tiles, nrhip_conv7x7_wgrad_workspace, ops_decoder._rows_per_wave) next to the case.

Branch reached <- shape, and the query that shows it:
  conv7_kernel<R>            tile counts <- nrhip_conv7x7_tiles; 1 / 2 / 3 / 4 column tiles, whole and ragged row tiles, R = 1, 2, 4
  conv7_wgrad_kernel         strips per image <- nrhip_conv7x7_wgrad_workspace: (45, 100, 17) six strips of 18 rows, the last
                             of 10; (2, 20, 50) 16 + 4 rows; W = 97, 130: 8 and 10 staging tasks for 7 waves (the unprefetched
                             loop, decoder_refs.wgrad_tasks restates the kernel's count: the ABI has no query for it)
  upsample_*                 (1, 257, 511): 4104 groups of 32 pixels > 4 x 1024 waves (forward, data gradient), 16-17 passes
                             per wave of the weight gradient's 256
  conv1x1_in_*               cin = 1, 5, 47 (ragged quarters and eighths), 48, 64; n across one and two 64-pixel workgroups
  rgb_bwd_kernel             n = 4099: five 1024-pixel blocks, the last with 3 pixels
  grad_amax_kernel           524,293 floats: 129 blocks asked, 128 launched, a 17th stride pass for the last five
  bn_bwd_reduce_kernel       1,048,579 pixels: 1025 blocks asked, 1024 launched
  colsum64 (bn_finalize)     n = 1 .. 1000 partial rows around the 16 slices and the 2-way unrolled loop
  whole decoder              rows_hi = 4 / 2 / 1 <- ops_decoder._rows_per_wave; hi-res width 120 <- wgrad_tasks

Observed on an MI355X, for the record only (largest err / bound of a bounded check; no bound is set from these):
  rgb_fwd 0.23; rgb_bwd grad_h 0.996, grad_weight 0.65 (at n = 1, six roundings against a bound of eleven), grad_bias 0.35
  bn_bwd grad_c 0.995, grad_gamma 0.016, grad_beta 0.026
  bn_finalize: at most 1.65 fp32 ulps over all coefficient rows and running statistics
  bn_act: bit-equal, no element of these inputs within 2^-30 of a rounding boundary
grad_h and grad_c are fp16 results: the bound's half-ulp term 2^-11 |ref| is reached by any correctly rounded value at the
bottom of its binade, so a ratio just under 1 is what a correct kernel gives; the accumulation terms behind it are spare."""
import ctypes as C

import pytest
import torch

import decoder_refs as DR

pytestmark = pytest.mark.gpu


def _D():
    from neurad_studio_amd import ops_decoder

    return ops_decoder


def _tiles(h, w, r):
    from neurad_studio_amd._lib import call

    t = C.c_int32(0)
    call("nrhip_conv7x7_tiles", h, w, r, C.byref(t))
    return t.value


def _wgrad_strips(b, h, w):
    from neurad_studio_amd._lib import call

    f = C.c_int64(0)
    call("nrhip_conv7x7_wgrad_workspace", b, h, w, C.byref(f))
    assert f.value % ((49 * 1024 + 32) * b) == 0
    return f.value // (49 * 1024 + 32) // b


def _note(what, value):
    print(f"[decoder-exact] {what}: {value:.3g}")


# ---- a. conv7x7 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 4])
def test_conv7x7_is_exact_in_both_pack_modes_with_exact_statistics(R):
    """one pixel; one ragged tile (4R - 1 rows, 31 columns); two tiles each way with one row / one column in the second;
    three column tiles with whole row tiles; four column tiles with a ragged row tile and two images"""
    D = _D()
    for B, H, W in DR.conv_shapes(R):
        c = DR.conv_case(B, H, W)
        tiles = _tiles(H, W, R)
        assert tiles == -(-W // 32) * -(-H // (4 * R))
        s1, s2 = DR.conv_tile_sums(c["out"], R)
        assert s1 < 2 ** 24 and s2 < 2 ** 24  # no per-workgroup partial can round
        x, g, w, bias = c["x"].cuda(), c["g"].cuda(), c["w"].cuda(), c["bias"].cuda()
        out, part = D.conv7x7(x, D.conv7x7_pack(w, 0), bias, stats=True, rows_per_wave=R)
        assert part.shape == (B * tiles, 64)
        DR.assert_equal(out, c["out"], f"conv7x7 R={R} {(B, H, W)} forward")
        plain, none = D.conv7x7(x, D.conv7x7_pack(w, 0), bias, rows_per_wave=R)
        assert none is None and torch.equal(plain, out)
        s, o = part.double().sum(0), out.double().reshape(-1, 32)
        assert torch.equal(s[:32], o.sum(0)) and torch.equal(s[32:], o.square().sum(0)), (R, B, H, W)
        dx, _ = D.conv7x7(g, D.conv7x7_pack(w, 1), None, rows_per_wave=R)
        DR.assert_equal(dx, c["dx"], f"conv7x7 R={R} {(B, H, W)} input gradient (pack mode 1)")


def test_conv7x7_pack_many_is_eight_single_packs():
    D = _D()
    g = torch.Generator(device="cuda").manual_seed(2)
    ws = [torch.randn((32, 32, 7, 7), device="cuda", generator=g) for _ in range(8)]
    many = D.conv7x7_pack_many(ws)
    for i, w in enumerate(ws):
        for m in (0, 1):
            assert torch.equal(many[i, m], D.conv7x7_pack(w, m)), (i, m)


# ---- b. conv7x7_wgrad --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DR.WGRAD_SHAPES)
def test_conv7x7_weight_gradient_is_exact(shape):
    D = _D()
    B, H, W = shape
    rps, spi = DR.wgrad_plan(B, H)
    assert _wgrad_strips(B, H, W) == spi
    if shape == (45, 100, 17):  # six strips of a 100-row image: 17..19 rows each, neither 16 nor H; 18 by the plan, last one 10
        assert spi == 6 and rps == 18 and H - 5 * rps == 10
    if shape == (2, 20, 50):
        assert spi == 2 and H - rps == 4  # ragged last strip
    assert (sum(DR.wgrad_tasks(W)) > 7) == (W in (97, 130))  # the unprefetched loop of wide rows
    scale = D.grad_scale(torch.tensor([0.0, -2.0 ** -7, 2.0 ** -9], device="cuda"))
    assert scale[:2].tolist() == [64.0, 2.0 ** -6]
    for sc, lsb in ((None, 1.0), (scale, 2.0 ** -6)):
        c = DR.wgrad_case(B, H, W, lsb=lsb)
        gw = torch.full((32, 32, 7, 7), c["prefill"], device="cuda")
        gb = torch.full((32,), c["prefill"], device="cuda")
        D.conv7x7_wgrad(c["x"].cuda(), c["g"].cuda(), gw, gb, sc)
        DR.assert_equal(gw, c["prefill"] + c["dw"] * lsb, f"conv7x7_wgrad {shape} weight, 1/S = {lsb}")
        DR.assert_equal(gb, c["prefill"] + c["db"] * lsb, f"conv7x7_wgrad {shape} bias, 1/S = {lsb}")


def test_conv7x7_weight_gradient_refuses_a_row_that_does_not_fit_in_lds():
    from neurad_studio_amd._lib import NeuradHipError

    D = _D()
    W = next(w for w in range(1, 4096) if DR.wgrad_lds_bytes(w) > 160 * 1024)
    assert DR.wgrad_lds_bytes(W - 1) <= 160 * 1024
    x = torch.zeros((1, 1, W, 32), device="cuda", dtype=torch.float16)
    gw = torch.zeros((32, 32, 7, 7), device="cuda")
    with pytest.raises(NeuradHipError, match="LDS"):
        D.conv7x7_wgrad(x, x, gw, None)
    assert float(gw.abs().max()) == 0.0  # nothing was launched


# ---- c. transposed convolution -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DR.UP_SHAPES + [DR.UP_SHAPE_CAPPED])
def test_transposed_convolution_is_exact(shape):
    D = _D()
    B, H, W = shape
    groups = -(-B * H * W // 32)
    if shape == DR.UP_SHAPE_CAPPED:  # forward / data gradient: > 1024 workgroups of 4 waves; weight gradient: 256 waves
        assert -(-groups // 4) > 1024 and groups > 16 * 256
    else:
        assert groups <= 256
    c = DR.up_case(B, H, W)
    x, g, w, bias = c["x"].cuda(), c["g"].cuda(), c["w"].cuda(), c["bias"].cuda()
    wup = D.upsample_pack(w)
    DR.assert_equal(D.upsample_fwd(x, wup, bias), c["out"], f"upsample_fwd {shape}")
    gw, gb = torch.full((32, 32, 3, 3), -5.0, device="cuda"), torch.full((32,), 7.0, device="cuda")
    DR.exact_fp32(c["dw"].abs() + 5, "prefilled weight gradient"), DR.exact_fp32(c["db"].abs() + 7, "prefilled bias gradient")
    dx = D.upsample_bwd(x, g, wup, gw, gb)
    DR.assert_equal(dx, c["dx"], f"upsample_bwd {shape} data gradient")
    DR.assert_equal(gw, c["dw"] - 5.0, f"upsample_bwd {shape} weight gradient")
    DR.assert_equal(gb, c["db"] + 7.0, f"upsample_bwd {shape} bias gradient")


# ---- d. first layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", DR.IN_CINS)
def test_first_layer_is_exact(cin):
    """cin splits in quarters (data gradient) and eighths (weight gradient) with ragged remainders; n around the 64-pixel
    workgroup and past two of them"""
    D = _D()
    for n in DR.IN_NS:
        c = DR.in_case(n, cin)
        feat, w, bias, dh = c["feat"].cuda(), c["w"].cuda(), c["bias"].cuda(), c["dh"].cuda()
        h = D.conv1x1_in_fwd(feat, w.reshape(32, cin, 1, 1), bias)
        DR.assert_equal(h, c["h"], f"conv1x1_in_fwd n={n} cin={cin}")
        gw, gb = torch.full((32, cin), 2.0, device="cuda"), torch.full((32,), -4.0, device="cuda")
        gf = D.conv1x1_in_bwd(feat, h, dh, w, gw, gb)
        DR.assert_equal(gf, c["dfeat"], f"conv1x1_in_bwd n={n} cin={cin} dfeat")
        DR.assert_equal(gw, c["dw"] + 2.0, f"conv1x1_in_bwd n={n} cin={cin} grad_weight")
        DR.assert_equal(gb, c["db"] - 4.0, f"conv1x1_in_bwd n={n} cin={cin} grad_bias")


def test_first_layer_refuses_65_input_channels_on_the_host():
    from neurad_studio_amd._lib import NeuradHipError

    D = _D()
    f, w, b = torch.zeros((3, 65), device="cuda"), torch.zeros((32, 65), device="cuda"), torch.zeros((32,), device="cuda")
    with pytest.raises(NeuradHipError, match="65 input channels"):
        D.conv1x1_in_fwd(f, w, b)
    with pytest.raises(NeuradHipError):
        D.conv1x1_in_bwd(f, torch.zeros((3, 32), device="cuda", dtype=torch.float16),
                         torch.zeros((3, 32), device="cuda", dtype=torch.float16), w, torch.zeros_like(w), b.clone())


# ---- e. last layer -------------------------------------------------------------------------------------------------------------
def test_last_layer_is_within_its_per_element_bounds():
    """n around one 256-pixel workgroup (forward) and around one 1024-pixel block (backward), then five blocks with a
    ragged tail of 3 pixels"""
    D = _D()
    g = torch.Generator().manual_seed(71)
    worst = dict(rgb=0.0, grad_h=0.0, grad_weight=0.0, grad_bias=0.0)
    for n in DR.RGB_NS:
        h = (torch.randn((1, 1, n, 32), generator=g) * 1.5).half()
        w, bias = torch.randn((3, 32), generator=g) * 0.3, torch.randn((3,), generator=g) * 0.1
        drgb = torch.randn((1, 1, n, 3), generator=g)
        gw0, gb0 = torch.randn((3, 32), generator=g), torch.randn((3,), generator=g)
        rgb = D.rgb_fwd(h.cuda(), w.cuda(), bias.cuda())
        s, a, abs_sum = DR.rgb_fwd(h, w, bias)
        worst["rgb"] = max(worst["rgb"], DR.assert_within(rgb, s, DR.rgb_fwd_bound(s, a, abs_sum), f"rgb_fwd n={n}"))
        gw, gb = gw0.cuda(), gb0.cuda()
        gh = D.rgb_bwd(h.cuda(), rgb, drgb.cuda(), w.cuda(), gw, gb)
        (dh, dw, db), (adh, adw, adb) = DR.rgb_bwd(h, rgb, drgb, w)
        worst["grad_h"] = max(worst["grad_h"], DR.assert_within(gh.reshape(n, 32), dh, DR.fp16_sum_bound(dh, adh, 8, DR.U32),
                                                                f"rgb_bwd n={n} grad_h"))
        for name, got, ref, mag, pre in (("grad_weight", gw, dw, adw, gw0), ("grad_bias", gb, db, adb, gb0)):
            want = ref + pre.double()
            bound = DR.gamma(n + 8) * mag + DR.U32 * (want.abs() + ref.abs())
            worst[name] = max(worst[name], DR.assert_within(got, want, bound, f"rgb_bwd n={n} {name}"))
    for k, v in worst.items():
        _note(f"rgb {k} err/bound", v)


# ---- f. grad_scale -------------------------------------------------------------------------------------------------------------
def test_grad_scale_finds_the_maximum_wherever_it_lies():
    """128 * 4096 + 5 floats: the 128-block cap is reached and the last five elements belong to a 17th grid-stride pass"""
    D = _D()
    n = 128 * 4096 + 5
    assert -(-n // 4096) > 128
    base = torch.rand((n,), generator=torch.Generator().manual_seed(81)) * 2.0 ** -12

    def check(edit, amax):
        t = base.clone()
        edit(t)
        got = D.grad_scale(t.cuda())[:2].cpu()
        assert torch.equal(got, torch.tensor(DR.expected_grad_scale(amax), dtype=torch.float32)), (got, amax)

    def put(i, v):
        def f(t):
            t[i] = v
        return f

    check(put(n - 1, -3.0), 3.0)             # only the 17th pass reads it
    check(put(128 * 256 + 77, 2.0 ** -3), 2.0 ** -3)  # the second pass of block 0
    check(put(0, 0.75), 0.75)
    check(lambda t: t.zero_(), 0.0)          # S = 1

    def nonfinite(t):
        t[5], t[n - 2], t[70000], t[9] = float("inf"), float("-inf"), float("nan"), 6.0
    check(nonfinite, 6.0)

    def tiny(t):
        t.zero_()
        t[12345] = -2.0 ** -70
    check(tiny, 2.0 ** -70)                  # e = 69 is clamped to 60
    assert DR.expected_grad_scale(2.0 ** -70) == (2.0 ** 60, 2.0 ** -60)


# ---- g. BatchNorm --------------------------------------------------------------------------------------------------------------
def test_bn_finalize_on_hand_made_partials_is_within_two_ulps():
    """n partial rows around the 16 slices and the 2-way unrolled loop of the column sum.  Signs are chosen so that neither
    shift = beta - mean scale nor a running statistic cancels: a bound in ulps of the RESULT is only meaningful then"""
    D = _D()
    g = torch.Generator().manual_seed(91)
    worst = 0.0
    for n in DR.BN_PARTIAL_NS:
        mean_c = torch.randn((32,), generator=g) * 2.0
        vals = torch.randn((n, 64, 32), generator=g) * (torch.rand((32,), generator=g) + 0.5) + mean_c
        part = torch.cat([vals.sum(1), vals.square().sum(1)], 1).float().contiguous()
        count = 64 * n
        sgn = torch.sign(DR.d64(part).sum(0)[:32]).float()
        gamma_ = torch.rand((32,), generator=g) + 0.5
        beta = -sgn * (torch.rand((32,), generator=g) + 0.1)
        rm0, rv0 = sgn * (torch.rand((32,), generator=g) + 0.1), torch.rand((32,), generator=g) + 0.5
        rm, rv = rm0.cuda(), rv0.cuda()
        coef = D.bn_finalize(part.cuda(), count, gamma_.cuda(), beta.cuda(), 1e-5, 0.1, rm, rv)
        ref, rm_ref, rv_ref = DR.bn_finalize(part, count, gamma_, beta, 1e-5, 0.1, rm0, rv0)
        for got, want, what in ((coef, ref, "coef"), (rm, rm_ref, "running_mean"), (rv, rv_ref, "running_var")):
            u = DR.ulps32(got, want)
            worst = max(worst, float(u.max()))
            assert (u <= 2.0).all(), (n, what, float(u.max()))
    _note("bn_finalize worst ulps", worst)


def _ew_inputs(npix, seed):
    g = torch.Generator().manual_seed(seed)
    c = (torch.randn((1, 1, npix, 32), generator=g) * 1.5 + 0.4).half()
    other = torch.randn((1, 1, npix, 32), generator=g).half()
    act = torch.relu(torch.randn((1, 1, npix, 32), generator=g)).half()
    coef = torch.stack([torch.rand((32,), generator=g) + 0.5, torch.randn((32,), generator=g) * 0.3,
                        torch.zeros(32), torch.ones(32)]).contiguous()
    return c, other, act, coef


@pytest.mark.parametrize("npix", DR.EW_PIXELS)
def test_bn_act_and_add_masked_replay_the_rounding_chain_bit_for_bit(npix):
    D = _D()
    c, other, act, coef = _ew_inputs(npix, 100 + npix)
    for skip in (None, other):
        want, exempt = DR.bn_act(c, coef, skip)
        got = D.bn_act(c.cuda(), coef.cuda(), None if skip is None else skip.cuda())
        DR.assert_equal(got, want, f"bn_act {npix} pixels, skip {skip is not None}", exempt)
        _note(f"bn_act {npix} exempt elements", float(exempt.sum()))
    want, _ = DR.add_masked(c, other, act)
    DR.assert_equal(D.add_masked(c.cuda(), other.cuda(), act.cuda()), want, f"add_masked {npix} pixels")


@pytest.mark.parametrize("npix", DR.EW_PIXELS + [DR.BN_BWD_PIXELS_CAPPED])
def test_bn_bwd_is_within_its_per_element_bounds(npix):
    """1024 * 1024 + 3 pixels: 4 (1024 * 1024 + 3) octets need 1025 blocks of 4096, the plan caps them at 1024"""
    D = _D()
    if npix == DR.BN_BWD_PIXELS_CAPPED:
        assert -(-4 * npix // 4096) > 1024
    c, dout, act, _ = _ew_inputs(npix, 200 + npix % 1000)
    g = torch.Generator().manual_seed(7)
    gamma_ = torch.rand((32,), generator=g) + 0.5
    mean, var, _ = DR.bn_stats(c)
    coef = torch.stack([torch.ones(32), torch.zeros(32), mean.float(), (var + 1e-5).rsqrt().float()]).contiguous()
    gg0, gb0 = torch.randn((32,), generator=g), torch.randn((32,), generator=g)
    gg, gb = gg0.cuda(), gb0.cuda()
    dc = D.bn_bwd(dout.cuda(), act.cuda(), c.cuda(), gamma_.cuda(), coef.cuda(), gg, gb)
    r = DR.bn_bwd(dout, act, c, gamma_, coef)
    _note(f"bn_bwd {npix} grad_c err/bound", DR.assert_within(dc, r["dc"], r["bound_dc"], f"bn_bwd {npix} grad_c"))
    for name, got, ref, b, pre in (("grad_gamma", gg, r["dgamma"], r["bound_dgamma"], gg0),
                                   ("grad_beta", gb, r["dbeta"], r["bound_dbeta"], gb0)):
        want = ref + pre.double()
        _note(f"bn_bwd {npix} {name} err/bound", DR.assert_within(got, want, b + DR.U32 * want.abs(), f"bn_bwd {npix} {name}"))


@pytest.mark.parametrize("R", [1, 4])
def test_batch_statistics_of_off_centre_channels(R):
    """channels with mean / std = 0, 3, 10, 30 (set through the convolution's bias): the statistics are E[x^2] - mean^2 from
    fp32 per-workgroup sums, and must stay within a quarter of an fp16 ulp of the fp64 statistics of the stored output:
    |rstd / rstd_ref - 1| <= 2^-12, |mean - mean_ref| <= 2^-12 std.
    Observed on an MI355X, worst channel per ratio, |rstd / rstd_ref - 1| and |mean - mean_ref| / std (2^-12 = 2.4e-4):
      R = 1   ratio 0: 4.7e-08, 4.9e-10   ratio 3: 1.9e-07, 1.3e-07   ratio 10: 1.4e-06, 3.6e-07   ratio 30: 2.4e-05, 7.0e-07
      R = 4   ratio 0: 4.7e-08, 1.0e-09   ratio 3: 3.5e-07, 1.4e-07   ratio 10: 6.1e-06, 3.6e-07   ratio 30: 2.7e-05, 7.0e-07"""
    D = _D()
    B, H, W = 3, 32, 32
    ratios = torch.tensor([0.0, 3.0, 10.0, 30.0]).repeat(8)
    g = torch.Generator().manual_seed(111)
    x = torch.randn((B, H, W, 32), generator=g).half()
    w = torch.randn((32, 32, 7, 7), generator=g) * 0.05
    m0, v0, _ = DR.bn_stats(DR.conv7_fwd(x, w.half()))
    bias = (ratios.double() * v0.sqrt() - m0).float()
    out, part = D.conv7x7(x.cuda(), D.conv7x7_pack(w.cuda(), 0), bias.cuda(), stats=True, rows_per_wave=R)
    coef = D.bn_finalize(part, B * H * W, torch.ones(32, device="cuda"), torch.zeros(32, device="cuda"), 1e-5, 0.1, None, None)
    mean, var, _ = DR.bn_stats(out)
    std = var.sqrt()
    assert ((mean / std - ratios.double()).abs() <= 0.05 * ratios.double() + 0.05).all()  # the ratios are the intended ones
    rstd_ref = 1.0 / torch.sqrt(var + float(torch.tensor(1e-5, dtype=torch.float32)))
    e_rstd = (DR.d64(coef[3]) / rstd_ref - 1).abs()
    e_mean = (DR.d64(coef[2]) - mean).abs() / std
    for k, ratio in enumerate((0, 3, 10, 30)):
        _note(f"off-centre R={R} ratio {ratio} rstd", float(e_rstd[k::4].max()))
        _note(f"off-centre R={R} ratio {ratio} mean", float(e_mean[k::4].max()))
    assert (e_rstd <= 2.0 ** -12).all(), e_rstd
    assert (e_mean <= 2.0 ** -12).all(), e_mean


# ---- h. the whole decoder ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_patches,patch,rows_hi,wide", [(30, (32, 32), 4, False), (128, (4, 11), 2, False),
                                                         (2, (8, 40), 1, True)])
def test_decoder_end_to_end_at_the_launch_plans_of_production(n_patches, patch, rows_hi, wide):
    """decode_rgb in train mode against the fp32 torch modules, torch autocast(fp16) as the yardstick with the margins of
    test_gpu_decoder.py, at 16-row and 8-row conv tiles and with the wide weight-gradient path inside the chain"""
    import copy

    from neurad_studio_amd.model_components.cnns import decode_rgb, make_rgb_decoder

    D = _D()
    ph, pw = patch
    assert D._rows_per_wave(3 * ph, 3 * pw, n_patches) == rows_hi
    assert (sum(DR.wgrad_tasks(3 * pw)) > 7) == wide
    torch.manual_seed(8)
    dec = make_rgb_decoder(48, 32, 3).cuda().train()
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    f = torch.randn((n_patches * ph * pw, 48), device="cuda")
    image = torch.rand((n_patches, 3 * ph, 3 * pw, 3), device="cuda")

    def run(mode):
        d = copy.deepcopy(dec)
        x = f.clone().requires_grad_()
        if mode == "hip":
            rgb = decode_rgb(d, x, patch)
        elif mode == "fp32":
            rgb = decode_rgb(d, x, patch, fused=False)
        else:
            with torch.autocast("cuda", dtype=torch.float16):
                rgb = decode_rgb(d, x, patch, fused=False)
        torch.nn.functional.mse_loss(rgb.float(), image).backward()
        return rgb.detach().float(), x.grad, {n: p.grad for n, p in d.named_parameters()}, dict(d.named_buffers())

    rgb_h, gx_h, gp_h, buf_h = run("hip")
    rgb_r, gx_r, gp_r, buf_r = run("fp32")
    rgb_a, gx_a, gp_a, _ = run("autocast")

    def rel(a, b):
        return float((a - b).norm() / (b.norm() + 1e-20))

    assert rgb_h.shape == (n_patches, 3 * ph, 3 * pw, 3)
    assert (rgb_h - rgb_r).abs().max() <= max(1.5 * float((rgb_a - rgb_r).abs().max()), 2e-3)
    assert rel(gx_h, gx_r) <= max(1.5 * rel(gx_a, gx_r), 5e-3)
    for n in gp_r:
        if n.endswith("main_branch.0.bias") or n.endswith("main_branch.3.bias"):
            continue  # a bias in front of BatchNorm has a zero gradient: only rounding noise on both sides
        assert rel(gp_h[n], gp_r[n]) <= max(1.5 * rel(gp_a[n], gp_r[n]), 5e-3), (n, rel(gp_h[n], gp_r[n]), rel(gp_a[n], gp_r[n]))
    for n in buf_r:
        if n.endswith("num_batches_tracked"):
            assert int(buf_h[n]) == int(buf_r[n]) == 1
        else:
            assert torch.allclose(buf_h[n], buf_r[n], rtol=2e-3, atol=2e-4), n
