"""tests/decoder_refs.py is right and sharp, shown on the CPU: its float64 references agree with the plain torch modules on
random data, its integer families keep every intermediate exactly representable at every shape the GPU tests use, and the
exact comparison flags each one-defect variant of a decoder kernel on at least one of those shapes."""
import pytest
import torch

import decoder_refs as DR


def _rand16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half()


def _close(a, b, what):
    assert (a - b).abs().max() <= 1e-12 * max(1.0, float(b.abs().max())), what


# ---- the references against the torch modules -----------------------------------------------------------------------------
def test_convolution_references_match_the_torch_modules():
    x, g = _rand16((2, 9, 37, 32), 1), _rand16((2, 9, 37, 32), 2)
    m = torch.nn.Conv2d(32, 32, 7, padding=3).double()
    xr = DR.nchw(x).requires_grad_()
    y = m(xr)
    y.backward(DR.nchw(g))
    w, b = m.weight.detach(), m.bias.detach()
    _close(DR.conv7_fwd(x, w, b), DR.nhwc(y.detach()), "conv forward")
    dx, dw, db = DR.conv7_grads(x, w, g)
    _close(dx, DR.nhwc(xr.grad), "conv input gradient")
    _close(dw, m.weight.grad, "conv weight gradient")
    _close(db, m.bias.grad, "conv bias gradient")
    # the input gradient is the forward convolution on flipped, transposed weights (pack mode 1)
    _close(DR.conv7_fwd(g, w.transpose(0, 1).flip(2, 3)), dx, "mode 1")


def test_transposed_convolution_references_match_the_torch_module():
    x, g = _rand16((2, 5, 7, 32), 3), _rand16((2, 15, 21, 32), 4)
    m = torch.nn.ConvTranspose2d(32, 32, 3, stride=3).double()
    xr = DR.nchw(x).requires_grad_()
    y = m(xr)
    y.backward(DR.nchw(g))
    _close(DR.up_fwd(x, m.weight.detach(), m.bias.detach()), DR.nhwc(y.detach()), "forward")
    for got, want, what in zip(DR.up_grads(x, m.weight.detach(), g), (DR.nhwc(xr.grad), m.weight.grad, m.bias.grad), "xwb"):
        _close(got, want, "transposed convolution gradient " + what)


def test_first_and_last_layer_references_match_the_torch_modules():
    cin, n = 47, 70
    feat, dh = _rand16((n, cin), 5).float(), _rand16((n, 32), 6)
    m = torch.nn.Sequential(torch.nn.Conv2d(cin, 32, 1), torch.nn.ReLU()).double()
    with torch.no_grad():
        m[0].weight.copy_(m[0].weight.half().double())
    fr = feat.double().requires_grad_()
    h = m(fr.t().reshape(1, cin, n, 1)).reshape(32, n).t()
    h.backward(dh.double())
    w, b = m[0].weight.detach().reshape(32, cin), m[0].bias.detach()
    _close(DR.in_fwd(feat, w, b), h.detach(), "first layer")
    for got, want in zip(DR.in_bwd(feat, w, h.detach(), dh), (fr.grad, m[0].weight.grad.reshape(32, cin), m[0].bias.grad)):
        _close(got, want, "first layer gradient")
    m = torch.nn.Sequential(torch.nn.Conv2d(32, 3, 1), torch.nn.Sigmoid()).double()
    with torch.no_grad():
        m[0].weight.copy_(m[0].weight.half().double())
    x, drgb = _rand16((n, 32), 7), _rand16((n, 3), 8).float()
    xr = x.double().requires_grad_()
    rgb = m(xr.t().reshape(1, 32, n, 1)).reshape(3, n).t()
    rgb.backward(drgb.double())
    w, b = m[0].weight.detach().reshape(3, 32), m[0].bias.detach()
    s, a, abs_sum = DR.rgb_fwd(x, w, b)
    _close(s, rgb.detach(), "last layer")
    assert (abs_sum >= a.abs() - 1e-12).all()
    (dh, dw, db), (adh, adw, adb) = DR.rgb_bwd(x, rgb.detach(), drgb, w)
    for got, want, mag in ((dh, xr.grad, adh), (dw, m[0].weight.grad.reshape(3, 32), adw), (db, m[0].bias.grad, adb)):
        _close(got, want, "last layer gradient")
        assert (mag >= got.abs() - 1e-12).all()


def test_batch_norm_references_match_the_torch_module():
    c = (_rand16((3, 6, 11, 32), 9).float() * 1.5 + 0.7).half()
    dout, skip = _rand16(c.shape, 10), _rand16(c.shape, 11)
    m = torch.nn.BatchNorm2d(32, eps=1e-5, momentum=0.125).double()  # an fp32 number
    with torch.no_grad():
        m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2), m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 2)
    rm, rv = m.running_mean.clone(), m.running_var.clone()
    cr = DR.nchw(c).requires_grad_()
    y = m(cr)
    v = DR.d64(c).reshape(-1, 32)
    part = torch.stack([torch.cat([v[i::4].sum(0), v[i::4].square().sum(0)]) for i in range(4)])  # 4 "workgroups"
    coef, rm2, rv2 = DR.bn_finalize(part, v.shape[0], m.weight, m.bias, 1e-5, 0.125, rm, rv)
    mean, var, unb = DR.bn_stats(c)
    assert torch.allclose(coef[2], mean, rtol=0, atol=1e-12) and torch.allclose(coef[3], (var + 1e-5).rsqrt(), rtol=1e-9)
    assert torch.allclose(rm2, m.running_mean, rtol=1e-7, atol=1e-9) and torch.allclose(rv2, m.running_var, rtol=1e-7)
    assert torch.allclose(DR.d64(c) * coef[0] + coef[1], DR.nhwc(y.detach()), rtol=0, atol=1e-6)  # shift holds an fp32 mean
    # backward, with the ReLU mask of the block's stored output
    out, _ = DR.bn_act(c, coef, skip)
    y.backward(DR.nchw(dout) * (DR.nchw(out) > 0))
    r = DR.bn_bwd(dout, out, c, m.weight, coef)
    assert torch.allclose(r["dc"], DR.nhwc(cr.grad), rtol=0, atol=1e-9)
    assert torch.allclose(r["dgamma"], m.weight.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(r["dbeta"], m.bias.grad, rtol=1e-9, atol=1e-9)
    # the rounding chain: one fp16 ulp around the unrounded value
    ref = torch.relu(DR.nhwc(y.detach()) + skip.double())
    assert ((out.double() - ref).abs() <= 2.0 ** -10 * ref.abs().clamp(min=1.0) + 2.0 ** -10 * skip.double().abs()).all()
    am, _ = DR.add_masked(c, dout, out)
    assert torch.equal(am, (c.float() + dout.float() * (out.float() > 0)).half())


def test_the_rounding_exemption_is_exactly_the_fp16_midpoints():
    t = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -35, 1.0 + 2.0 ** -11 + 2.0 ** -20, 3.0 * 2.0 ** -25, 0.0, 1.0,
                      -(1024.0 + 0.5)], dtype=torch.float64)
    d = DR._fp16_midpoint_distance(t) <= 2.0 ** -30
    assert d.tolist() == [True, True, False, True, False, False, True]
    with pytest.raises(ValueError):
        DR.rounding_exempt(t, "midpoints")
    # one rounding, not two: just below a tie whose fp32 rounding is the tie itself
    t = torch.tensor([1.0 + 3 * 2.0 ** -11 - 2.0 ** -30, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24 * 1.5, 2.0 ** -24 * 0.5, 2047.5, -0.3],
                     dtype=torch.float64)
    assert DR.round_to_fp16(t).tolist() == [1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, 2.0 ** -23, 0.0, 2048.0, -0.300048828125]
    assert t.float().half()[0].item() == 1.0 + 2.0 ** -9
    r = (torch.randn(100000, generator=torch.Generator().manual_seed(3)) * 3).double()  # fp32 numbers: torch rounds them once
    assert torch.equal(DR.round_to_fp16(r), r.float().half())


def test_checkers_report_and_bounds_behave():
    ref = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    assert DR.assert_within(ref + 0.25, ref, 0.5, "x") == 0.5
    with pytest.raises(AssertionError, match=r"2 of 6 .* first at \(0, 2\): got 3.0, want 2.0, bound 5.000e-01"):
        DR.assert_within(ref + torch.tensor([0.0, 0.0, 1.0]), ref, 0.5, "x")
    with pytest.raises(AssertionError):
        DR.assert_within(ref * float("nan"), ref, 0.5, "nan")
    with pytest.raises(AssertionError, match=r"1 of 6 .* first at \(1, 0\)"):
        DR.assert_equal((ref + torch.tensor([[0.0], [1.0]]) * torch.tensor([1.0, 0, 0])).half(), ref, "x")
    assert DR.ulps32(torch.tensor([1.0 + 2.0 ** -22]), torch.tensor([1.0], dtype=torch.float64)).item() == 2.0
    assert DR.expected_grad_scale(2.0 ** -7) == (64.0, 2.0 ** -6) and DR.expected_grad_scale(0.0) == (1.0, 1.0)
    assert DR.expected_grad_scale(0.75) == (1.0, 1.0) and DR.expected_grad_scale(2.0 ** -70) == (2.0 ** 60, 2.0 ** -60)
    with pytest.raises(ValueError):
        DR.exact_fp16(torch.tensor([2049.0]), "x")
    with pytest.raises(ValueError):
        DR.exact_fp32(torch.tensor([2.0 ** 18]), "x", lsb=2.0 ** -6)


# ---- the integer families stay representable at every shape the GPU tests use -----------------------------------------------
def test_integer_families_are_exactly_representable_at_every_listed_shape():
    for R in (1, 2, 4):
        for shape in DR.conv_shapes(R):
            c = DR.conv_case(*shape)
            assert torch.equal(c["out"], c["out"].half().double()) and torch.equal(c["dx"], c["dx"].half().double())
            s1, s2 = DR.conv_tile_sums(c["out"], R)
            assert s1 < 2 ** 24 and s2 < 2 ** 24, (shape, R, s1, s2)
    for shape in DR.WGRAD_SHAPES:
        for lsb in (1.0, 2.0 ** -6):
            c = DR.wgrad_case(*shape, lsb=lsb)
            assert torch.equal(c["dw"], c["dw"].float().double())
    for shape in DR.UP_SHAPES + [DR.UP_SHAPE_CAPPED]:
        c = DR.up_case(*shape)
        assert torch.equal(c["dw"], c["dw"].float().double()) and torch.equal(c["db"], c["db"].float().double())
    for n in DR.IN_NS:
        for cin in DR.IN_CINS:
            c = DR.in_case(n, cin)
            assert torch.equal(c["dw"], c["dw"].float().double())


# ---- one-defect variants ----------------------------------------------------------------------------------------------------
def _flagged(got, want):
    try:
        DR.assert_equal(got.to(want.dtype), want, "variant")
    except AssertionError:
        return True
    return False


def _all_conv_shapes():
    return sorted({s for R in (1, 2, 4) for s in DR.conv_shapes(R)})


def _conv_tilewise(x, w, bias, drop_halo):
    """the forward convolution tile by tile (32 output columns from 38 staged ones); DEFECT: the last halo column of a tile
    is read as zero"""
    B, H, W, _ = x.shape
    xp = torch.nn.functional.pad(DR.d64(x), (0, 0, 3, 3 + 32))
    out = torch.empty((B, H, W, 32), dtype=torch.float64)
    for x0 in range(0, W, 32):
        tile = xp[:, :, x0:x0 + 38].clone()
        if drop_halo:
            tile[:, :, 37] = 0
        y = torch.nn.functional.conv2d(tile.permute(0, 3, 1, 2), DR.d64(w), DR.d64(bias), padding=(3, 0))
        out[:, :, x0:x0 + 32] = y.permute(0, 2, 3, 1)[:, :, :min(32, W - x0)]
    return out


def test_forward_convolution_defects_are_flagged():
    c = DR.conv_case(2, 7, 97)
    x, w, b, g = c["x"], c["w"], c["bias"], c["g"]
    assert not _flagged(_conv_tilewise(x, w, b, False), c["out"])
    hits = {"transposed taps": [], "unflipped weights": [], "halo column": [], "channel pairs": []}
    swap = torch.arange(32) ^ 1
    for shape in _all_conv_shapes():
        c = DR.conv_case(*shape)
        x, w, b, g = c["x"], c["w"], c["bias"], c["g"]
        for name, got, want in (("transposed taps", DR.conv7_fwd(x, w.transpose(2, 3), b), c["out"]),
                                ("unflipped weights", DR.conv7_fwd(g, w.transpose(0, 1)), c["dx"]),
                                ("halo column", _conv_tilewise(x, w, b, True), c["out"]),
                                ("channel pairs", c["out"][..., swap], c["out"])):
            if _flagged(got.half(), want.half()):
                hits[name].append(shape)
    assert all(hits.values()), hits
    assert all(s[2] > 34 for s in hits["halo column"])  # only where a tile's last halo column is inside the image


def test_weight_gradient_defects_are_flagged():
    hits = []
    for shape in DR.WGRAD_SHAPES:
        c = DR.wgrad_case(*shape)
        B, H, W = shape
        rps, spi = DR.wgrad_plan(B, H)
        g = c["g"].clone()
        for s in range(spi):  # DEFECT: the last image row of every strip never reaches the accumulators
            g[:, min(H, (s + 1) * rps) - 1] = 0
        _, dw, db = DR.conv7_grads(c["x"], torch.zeros(32, 32, 7, 7), g)
        if _flagged(dw.float(), c["dw"].float()):
            hits.append(shape)
    assert (45, 100, 17) in hits and (2, 20, 50) in hits, hits
    assert DR.wgrad_plan(45, 100) == (18, 6) and DR.wgrad_plan(2, 20) == (16, 2) and DR.wgrad_plan(1, 5) == (5, 1)


def test_upsampling_defects_are_flagged():
    hits = []
    for shape in DR.UP_SHAPES:
        c = DR.up_case(*shape)
        B, H, W = shape
        n = B * H * W
        out = c["out"].clone().reshape(B, H, 3, W, 3, 32).permute(0, 1, 3, 2, 4, 5).reshape(n, 9 * 32)
        out[n // 32 * 32:] = 0  # DEFECT: the ragged last group of 32 input pixels writes nothing
        out = out.reshape(B, H, W, 3, 3, 32).permute(0, 1, 3, 2, 4, 5).reshape(B, 3 * H, 3 * W, 32)
        if _flagged(out, c["out"]):
            hits.append(shape)
    assert set(hits) == {s for s in DR.UP_SHAPES if (s[0] * s[1] * s[2]) % 32}, hits
    # DEFECT: a wave's accumulators are overwritten by its later passes (256 waves, group k goes to wave k % 256)
    c = DR.up_case(*DR.UP_SHAPE_CAPPED)
    B, H, W = DR.UP_SHAPE_CAPPED
    n = B * H * W
    groups = -(-n // 32)
    assert groups > 15 * 256
    x = c["x"].clone().reshape(n, 32)
    x[: max(0, groups - 256) * 32] = 0
    _, dw, _ = DR.up_grads(x.reshape(B, H, W, 32), c["w"], c["g"])
    assert _flagged(dw.float(), c["dw"].float())
    c = DR.up_case(2, 10, 12)  # one pass per wave: the defect cannot show
    assert -(-240 // 32) <= 256


def test_first_layer_remainder_defect_is_flagged():
    hits = []
    for cin in DR.IN_CINS:
        c = DR.in_case(130, cin)
        dw = c["dw"].clone()
        dw[:, cin // 8 * 8:] = 0  # DEFECT: the inputs behind the last whole eighth are dropped
        if _flagged(dw.float(), c["dw"].float()):
            hits.append(cin)
    assert hits == [1, 5, 47], hits
