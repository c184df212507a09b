"""Compositing at a trained scene's numerics: sharp surfaces, alphas of exactly 1 and 1 - 2^-24, transmittance that
underflows, sigma * delta past exp's range, zero-length bins and a sky bin far away.  Every kernel is held to a float64
torch reference PER ELEMENT, |got - ref| <= atol + rtol * mag, where mag is the float64 size of what the kernel's fp32
arithmetic adds up for that element (a sum of magnitudes, not the possibly cancelling result) and rtol counts the fp32
roundings along the longest chain (S samples of a scan, C channels of a dot product).  atol is below fp32's normal range:
a product that passes through the subnormals (< 2^-126) keeps no relative precision, and nothing that small is a
gradient anyone uses.  A whole-tensor rel-L2 is dominated by the largest entries and would not see one wrong ray."""
import numpy as np
import pytest

import neurad_oracle as O
import synth
from builders import sample_rays, shape_params
from composite_refs import ref_composite
from gpu_util import dev, host64, to_spec
from gpu_util import ops  # noqa: F401  (fixture)
from sharp_refs import R, SAMPLES, TINY, U, check, ref_alpha, ref_density, sharp_alphas, sharp_bins

pytestmark = pytest.mark.gpu

# ---- the compositing ops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SAMPLES)
def test_render_weight_from_alpha_saturated(ops, S):
    """C1 alpha mode (WeightFromAlphaFn / the nerfacc shim).  The backward must equal torch's cumprod backward where
    alpha == 1 exactly: T_k = 0 behind it, and dividing sum_{k>i} G_k T_k by 1 - alpha_i can not bring back the term
    -T_i sum_{k>i} G_k prod_{i<j<k}(1 - alpha_j) that the reference keeps."""
    a = sharp_alphas(S, seed=10 + S)
    gw, gt = synth.normal((R, S), 20 + S), synth.normal((R, S), 30 + S)
    w, t = ops.render_weight_from_alpha(dev(a))
    rw, rt, rga, mag = ref_alpha(a, gw, gt)
    rtol = 2 * (S + 2) * U  # S - 1 products per transmittance, one more for the weight
    check(host64(w), rw, TINY + rtol * rw, "weights")
    check(host64(t), rt, TINY + rtol * rt, "trans")
    # the forward is one product scan: exact zeros stay exact zeros, and the ray without special values is untouched
    assert (host64(w)[a == 0] == 0).all() and (host64(t)[:, 1:][np.cumsum(a == 1, -1)[:, :-1] > 0] == 0).all()
    ga = host64(ops.render_weight_from_alpha_bwd(dev(a), dev(gw), dev(gt)))
    gscale = np.abs(gw).max(-1, keepdims=True) + np.abs(gt).max(-1, keepdims=True)
    # T_k's S products, the term's product, the S-term suffix sum, the division, the subtraction
    check(ga, rga, 2.0 ** -100 * gscale + 4 * (S + 8) * U * mag, "dL/dalpha")
    ga0 = host64(ops.render_weight_from_alpha_bwd(dev(a), dev(gw)))  # grad_t = None
    _, _, rga0, mag0 = ref_alpha(a, gw, np.zeros_like(gt))
    check(ga0, rga0, 2.0 ** -100 * gscale + 4 * (S + 8) * U * mag0, "dL/dalpha (no grad_t)")


@pytest.mark.parametrize("S", SAMPLES)
def test_render_weight_from_density_saturated(ops, S):
    """C1 density mode and S3 (weights_from_density): sigma * delta past 88, zero-length bins, a sky bin at 1e10"""
    st, en, sig, _ = sharp_bins(S, seed=40 + S)
    delta = en - st  # fp32, as the kernel forms it
    gw = synth.normal((R, S), 50 + S)
    rw, rt, ra, rgs, fscale, gscale = ref_density(delta, sig, gw)
    w, t, a = ops.render_weight_from_density(dev(st), dev(en), dev(sig))
    check(host64(w), rw, TINY + fscale, "weights")
    check(host64(t), rt, TINY + fscale, "trans")
    check(host64(a), ra, TINY + 4 * U, "alphas")
    gs = host64(ops.render_weight_from_density_bwd(dev(st), dev(en), dev(sig), dev(gw)))
    atol = TINY * (delta.astype(np.float64) + 1) * np.abs(gw).max(-1, keepdims=True)
    check(gs, rgs, atol + gscale, "dL/dsigma")
    w2 = host64(ops.weights_from_density(dev(delta), dev(sig)))
    check(w2, rw, TINY + fscale, "weights_from_density")
    gs2 = host64(ops.weights_from_density_bwd(dev(delta), dev(sig), dev(gw)))
    check(gs2, rgs, atol + gscale, "weights_from_density_bwd")


@pytest.mark.parametrize("S", SAMPLES)
def test_prop_weights_saturated(ops, S):
    """S3 + render_depth_simple from the bin edges (the proposal rounds), forward and backward"""
    _, _, dens, e = sharp_bins(S, seed=60 + S)
    e = e.copy()
    e[::3, -1] = 1e4  # (a sky edge of 1e10 would make the depth's midpoints the whole story)
    delta = e[:, 1:] - e[:, :-1]
    mid = ((e[:, :-1] + e[:, 1:]) / np.float32(2)).astype(np.float64)
    gw, gd = synth.normal((R, S), 70 + S), synth.normal((R, 1), 71 + S)
    rw, _, _, _, fscale, _ = ref_density(delta, dens, gw)
    w, depth = ops.prop_weights_fwd(dev(e), dev(dens))
    check(host64(w), rw, TINY + fscale, "weights")
    rdepth = (rw * mid).sum(-1, keepdims=True)
    check(host64(depth), rdepth, TINY + ((fscale + S * U * rw) * np.abs(mid)).sum(-1, keepdims=True), "depth")
    # backward: the upstream of each weight is gw + g_depth * mid
    G = gw.astype(np.float64) + gd.astype(np.float64) * mid
    _, _, _, rgs, _, gscale = ref_density(delta, dens, G)
    _, _, _, _, _, gscale2 = ref_density(delta, dens, np.abs(gw) + np.abs(gd * mid))
    gs = host64(ops.prop_weights_bwd(dev(e), dev(dens), dev(gw), dev(gd)))
    atol = TINY * (delta.astype(np.float64) + 1) * np.abs(G).max(-1, keepdims=True)
    check(gs, rgs, atol + gscale + gscale2, "dL/ddensity")


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("C", [32, 3])
def test_composite_saturated(ops, S, C):
    """C2 on weights of saturated rays: acc == 1 to the last bit, the sky residual is 0 or -ulp, a zero weight tail"""
    a = sharp_alphas(S, seed=80 + S)
    w = O.render_weight_from_alpha(a)[0]
    st, en, _, _ = sharp_bins(S, seed=81 + S)
    feats = synth.normal((R, S, C), 82 + S)
    w2, rf, rd, ra, mid = ref_composite(w, feats, st, en)
    of, od, oa = ops.composite_fwd(dev(w), dev(feats), dev(st), dev(en))
    sw = w.astype(np.float64).sum(-1, keepdims=True)
    check(host64(oa), ra, 2 * S * U * sw, "acc")
    absf = np.abs(feats.astype(np.float64))
    fb = 2 * (S + 4) * U * ((np.abs(w2)[..., None] * absf).sum(1) + (1 + sw) * absf[:, -1])
    check(host64(of), rf, fb, "features")
    check(host64(od), rd, 2 * (S + 2) * U * (np.abs(w2[:, :-1]) * np.abs(mid[:, :-1])).sum(-1, keepdims=True), "depth")
    gF, gD, gA = synth.normal((R, C), 83), synth.normal((R, 1), 84), synth.normal((R, 1), 85)
    gw, gf = ops.composite_bwd(dev(w), dev(feats), dev(st), dev(en), dev(gF), dev(gD), dev(gA))
    # df_sc = w2_s gF_c ; dw_s = q_s - q_{S-1} + g_acc + g_depth mid_s [s < S-1],  q_s = sum_c gF_c f_sc
    gF64 = gF.astype(np.float64)
    rgf = w2[..., None] * gF64[:, None, :]
    check(host64(gf), rgf, 2 * (S + 2) * U * (np.abs(rgf) + (1 + sw)[..., None] * np.abs(gF64)[:, None, :]), "d features")
    q = (feats.astype(np.float64) * gF64[:, None, :]).sum(-1)
    qm = (absf * np.abs(gF64)[:, None, :]).sum(-1)
    dm = np.where(np.arange(S)[None] < S - 1, mid, 0.0)
    rgw = q - q[:, -1:] + gA + gD * dm
    check(host64(gw), rgw, 2 * (C + 4) * U * (qm + qm[:, -1:] + np.abs(gA) + np.abs(gD * dm)), "d weights")


@pytest.mark.parametrize("pair", ["0", "1"])
@pytest.mark.parametrize("S", SAMPLES[1:])  # (sdf_render wants S >= 2: the sky sample and at least one in front of it)
def test_sdf_render_saturated(ops, switches, S, pair):
    """SDF head + C1 + C2 (train_fused.hip sdf_render_*), one and two rays per wave (NRHIP_SDF_RENDER_PAIR: S <= 32, C = 32).
    The float64 reference composites the kernel's own fp32 alphas (checked against a float64 sigmoid first): a sharp
    beta makes alpha = sigmoid(-sdf beta) round to exactly 1 in fp32 where float64 still sees 1 - 1e-9, and the gradient
    through alpha (1 - alpha) is then exactly 0 in both."""
    switches.set("NRHIP_SDF_RENDER_PAIR", pair)
    C = 32
    beta_raw = 180.0
    sdf = (synth.normal((R, S), 90 + S) * 0.2).astype(np.float32)
    sdf[1, S // 3:] = -1.0  # deep inside: alpha == 1 exactly for the rest of the ray
    sdf[2, :] = 0.0  # alpha = 1/2 throughout: transmittance halves per sample
    sdf[3, S // 2:] = -0.09  # alpha = 1 - 2^-24 .. 1 (x beta ~ 16.3)
    sdf[4, :] = 1.0  # empty space: alpha == 0 in fp32 (sigmoid(-180) is subnormal-small)
    feats = synth.normal((R, S, C), 91 + S)
    e = np.cumsum(synth.uniform((R, S + 1), 0.01, 1.0, 92 + S), -1).astype(np.float32)
    e[::2, -1] = 1e10  # sky
    beta = dev(np.array([beta_raw], np.float32))
    a, w_ns, out, depth, acc = ops.sdf_render_fwd(dev(sdf), beta, 0.1, dev(feats), dev(e))
    b = beta_raw + 0.1
    a32 = host64(a)
    x = -sdf.astype(np.float64) * np.float64(np.float32(b))
    sig = 1 / (1 + np.exp(-x))
    # fp32 sigmoid of the fp32 product: the product's rounding moves x by u|x|, the sigmoid's own by a few ulp
    # (an fp32 exp of a rounded x: 3 |x| u relative on exp(-x), i.e. on the smaller of sigma and 1 - sigma)
    check(a32, sig, TINY + 4 * U * sig + sig * (1 - sig) * 3 * np.abs(x) * U, "alpha")
    # compositing of those alphas, float64
    rw, rT, _, _ = ref_alpha(a32.astype(np.float32), np.zeros((R, S)), np.zeros((R, S)))
    st, en = e[:, :-1], e[:, 1:]
    w2, rf, rd, ra, mid = ref_composite(rw, feats, st, en)
    check(host64(w_ns), rw[:, :-1], TINY + 2 * (S + 2) * U * rw[:, :-1], "weights_ns")
    check(host64(acc), rw.sum(-1, keepdims=True), TINY + 2 * (S + 2) * U * rw.sum(-1, keepdims=True), "acc")
    absf = np.abs(feats.astype(np.float64))
    sw = rw.sum(-1, keepdims=True)
    check(host64(out), rf, 4 * (S + 4) * U * ((np.abs(w2)[..., None] * absf).sum(1) + (1 + sw) * absf[:, -1]), "features")
    check(host64(depth), rd, TINY + 4 * (S + 4) * U * (rw[:, :-1] * np.abs(mid[:, :-1])).sum(-1, keepdims=True), "depth")
    # backward: upstream on features, depth, acc and the weights without the sky sample
    gF, gD, gA = synth.normal((R, C), 93), synth.normal((R, 1), 94), synth.normal((R, 1), 95)
    gWns = synth.normal((R, S - 1), 96)
    gfeat, gsdf, gbeta = ops.sdf_render_bwd(dev(sdf), beta, 0.1, a, dev(feats), dev(e), dev(gF), dev(gD), dev(gA),
                                             dev(gWns))
    gF64 = gF.astype(np.float64)
    rgf = w2[..., None] * gF64[:, None, :]
    check(host64(gfeat), rgf, 4 * (S + 4) * U * (np.abs(rgf) + (1 + sw)[..., None] * np.abs(gF64)[:, None, :]), "d features")
    # dL/dw_s (as composite_bwd), then the alpha-mode backward, then sigmoid' = alpha (1 - alpha) and x = -sdf beta
    q = (feats.astype(np.float64) * gF64[:, None, :]).sum(-1)
    qm = (absf * np.abs(gF64)[:, None, :]).sum(-1)
    dm = np.where(np.arange(S)[None] < S - 1, mid, 0.0)
    gwn = np.concatenate([gWns.astype(np.float64), np.zeros((R, 1))], -1)
    gw = q - q[:, -1:] + gA + gD * dm + gwn
    gw_mag = qm + qm[:, -1:] + np.abs(gA) + np.abs(gD * dm) + np.abs(gwn)
    _, _, rga, _ = ref_alpha(a32.astype(np.float32), gw, np.zeros((R, S)))
    _, _, _, mag = ref_alpha(a32.astype(np.float32), gw_mag, np.zeros((R, S)))
    a64 = a32.astype(np.float64)
    ds = a64 * (1 - a64)
    rgsdf = -rga * ds * b
    bound = (2.0 ** -100 * np.abs(gw_mag).max(-1, keepdims=True) + 4 * (S + C + 8) * U * mag) * ds * b
    check(host64(gsdf), rgsdf, bound, "d sdf")
    # d beta_raw = sum over rays and samples of -ds * x / beta ... = sum(rga * ds * (-sdf)) (beta_raw > 0)
    rgb = float((rga * ds * -sdf.astype(np.float64)).sum())
    gb_bound = float((bound / b * np.abs(sdf)).sum()) + 2 * R * S * U * float((np.abs(rga * ds * sdf)).sum())
    check(host64(gbeta).reshape(()), rgb, gb_bound + 1e-30, "d beta")
    assert np.isfinite(host64(gsdf)).all()


@pytest.mark.parametrize("S", [16, 65])
def test_sdf_render_density_head_saturated(ops, S):
    """sdf_render with beta = None (the density head): sigma = trunc_exp(x) with x up to 12, alpha rounds to 1"""
    C = 32
    x = synth.uniform((R, S), -8.0, 12.0, 100 + S)
    feats = synth.normal((R, S, C), 101 + S)
    e = np.cumsum(synth.uniform((R, S + 1), 0.0, 0.5, 102 + S), -1).astype(np.float32)
    e[:, 3] = e[:, 2]  # one zero-length bin per ray (S > 3)
    e[::2, -1] = 1e10
    a, w_ns, out, depth, acc = ops.sdf_render_fwd(dev(x), None, 0.0, dev(feats), dev(e))
    delta = (e[:, 1:] - e[:, :-1]).astype(np.float64)
    sd = np.exp(x.astype(np.float64)) * delta
    ra = -np.expm1(-sd)
    # fp32 exp(x) (relative 2u) times delta: sd off by 3u sd, alpha by (1 - alpha) 3u sd
    check(host64(a), ra, TINY + 4 * U * ra + (1 - ra) * 3 * U * sd, "alpha")
    a32 = host64(a)
    rw, _, _, _ = ref_alpha(a32.astype(np.float32), np.zeros((R, S)), np.zeros((R, S)))
    check(host64(acc), rw.sum(-1, keepdims=True), TINY + 2 * (S + 2) * U * rw.sum(-1, keepdims=True), "acc")
    gF, gD, gA = synth.normal((R, C), 103), synth.normal((R, 1), 104), synth.normal((R, 1), 105)
    gfeat, gx, gbeta = ops.sdf_render_bwd(dev(x), None, 0.0, a, dev(feats), dev(e), dev(gF), dev(gD), dev(gA), None)
    assert gbeta is None
    st, en = e[:, :-1], e[:, 1:]
    w2, _, _, _, mid = ref_composite(rw, feats, st, en)
    gF64 = gF.astype(np.float64)
    absf = np.abs(feats.astype(np.float64))
    q = (feats.astype(np.float64) * gF64[:, None, :]).sum(-1)
    qm = (absf * np.abs(gF64)[:, None, :]).sum(-1)
    dm = np.where(np.arange(S)[None] < S - 1, mid, 0.0)
    gw = q - q[:, -1:] + gA + gD * dm
    gw_mag = qm + qm[:, -1:] + np.abs(gA) + np.abs(gD * dm)
    _, _, rga, _ = ref_alpha(a32.astype(np.float32), gw, np.zeros((R, S)))
    _, _, _, mag = ref_alpha(a32.astype(np.float32), gw_mag, np.zeros((R, S)))
    # alpha = 1 - exp(-e^x delta): d alpha / dx = (1 - alpha) sigma delta, with trunc_exp's exp(clamp(x, -15, 15))
    a64 = a32.astype(np.float64)
    chain = (1 - a64) * delta * np.exp(np.clip(x.astype(np.float64), -15, 15))
    bound = (2.0 ** -100 * gw_mag.max(-1, keepdims=True) + 4 * (S + C + 8) * U * mag) * chain
    check(host64(gx), rga * chain, bound, "d x")


# ---- the fused render kernels at sharp beta -------------------------------------------------------------------------
FUSED = [(16, 2, 64), (8, 4, 32), (4, 8, 64), (1, 4, 32), (4, 2, 64), (4, 4, 32), (8, 2, 64)]  # (L, F, H)


def _sharp_field(L, F, H, head, half, rays):
    use_sdf = head != "density"
    p = shape_params(L, F, H, use_sdf, half=half)
    p.geo_b[1] = p.geo_b[1].copy()
    if use_sdf:
        p.beta = float(head)  # the learned beta of a trained scene: 20 .. 2000
        # move the surface into the rays: half of the samples end up at sdf < -1, where sigmoid(-sdf beta) is exactly 1
        # in fp32 for every beta here
        p.geo_b[1][0] -= np.float32(np.median(O.field_fwd(p, *rays)["sdf"]) + 1.0)
    else:
        p.geo_b[1][0] += np.float32(6.0)  # a density logit shifted up: sigma ~ e^6 and more, most rays go opaque
    return p


def per_ray_bounds(alpha_ref, dalpha, S):
    """|w_s - w_ref_s| <= sum_{j<=s} |alpha_j - alpha_ref_j| + rounding: every weight is alpha_s prod_{j<s}(1 - alpha_j), a
    product of factors in [0, 1], so an error in one factor moves it by at most that error.  The per-ray budget is the sum
    over the ray of the alpha errors the field's fp32 MLP leaves (measured per sample below) and S roundings."""
    return np.cumsum(dalpha, -1) + 4 * (S + 4) * U


@pytest.mark.parametrize("order", [False, True], ids=["batch", "ordered"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("head", ["20", "200", "2000", "density"])
@pytest.mark.parametrize("shape", FUSED, ids=[f"{l}x{f}" for l, f, _ in FUSED])
def test_render_fwd_sharp_surfaces(ops, shape, head, half, order):
    """render_fwd (composited) and field_fwd (per sample) of every fused grid shape at a trained scene's beta, against
    O.render_rays PER RAY.  The alphas of the per-sample path are checked against the oracle's with a beta-aware bound
    (d alpha / d sdf = beta alpha (1 - alpha) times the fp32 sdf error), and their measured error is the budget that the
    composited weights, accumulation, depth and features of each ray are held to."""
    L, F, H = shape
    Rr, S = 37, 48
    o, d, area, s, e, eu = sample_rays(Rr, S, seed=L * 10 + F, fars=60.0)
    p = _sharp_field(L, F, H, head, half, (o, d, area, s, e))
    fs = to_spec(ops, p, half=half)
    ref = O.render_rays(p, o, d, area, s, e)
    do, dd, da = dev(o), dev(d), dev(area)
    edges = dev(eu)
    kw = {"order": ops.ray_order(do, dd, p.static_scale)} if order else {}
    feats, depth, acc, w = (host64(v) for v in ops.render_fwd(fs, do, dd, da, edges[:, :-1], edges[:, 1:],
                                                              return_weights=True, **kw))
    f2, sdf2, head2 = ops.field_fwd(fs, do, dd, da, dev(s), dev(e))
    rw = ref["weights"].astype(np.float64)
    if p.use_sdf:
        beta = abs(p.beta) + p.beta_min
        ra = ref["alpha"].astype(np.float64)
        rsdf = ref["sdf"].reshape(Rr, S).astype(np.float64)
        got_sdf = host64(sdf2).reshape(Rr, S)
        # the geometry MLP in fp32 against the oracle's fp32: a few 1e-6 of the layer's magnitude
        sdf_tol = 1e-5 * (1 + np.abs(rsdf))
        check(got_sdf, rsdf, sdf_tol, "sdf")
        got_a = host64(head2).reshape(Rr, S)
        # alpha's sensitivity to sdf is beta alpha (1 - alpha) <= beta / 4; the mean-value bound with the larger of the two
        # alphas' alpha (1 - alpha) would need the kernel's; beta / 4 * sdf_tol caps it where the sigmoid turns
        slope = beta * np.maximum(ra * (1 - ra), 0.25 * (np.abs(-rsdf * beta) < 40))
        check(got_a, ra, TINY + 4 * U + slope * sdf_tol * 2, "alpha")
        sat = (ra == 1.0).any(-1).mean()
    else:
        ra = 1 - np.exp(-ref["density"].reshape(Rr, S).astype(np.float64) * (e - s))
        got_a = None
        sat = (ref["accumulation"][:, 0] > 1 - 1e-6).mean()
    assert sat > 0.5, f"only {sat:.2f} of the rays saturate"
    if got_a is None:  # density head: sigma from the kernel's per-sample head, alpha as render_weight_from_density
        rden = ref["density"].reshape(Rr, S).astype(np.float64)
        got_den = host64(head2).reshape(Rr, S)
        # sigma = exp(x): the geometry output's fp32 error (as sdf_tol above) is a relative error of sigma
        check(got_den, rden, TINY + rden * np.expm1(1e-5 * (1 + np.abs(np.log(np.maximum(rden, TINY))))), "density")
        got_a = 1 - np.exp(-got_den * (e - s).astype(np.float64))
    dalpha = np.abs(got_a - ra)
    assert np.isfinite(dalpha).all()
    wb = per_ray_bounds(ra, dalpha, S) + 2 * S * U
    check(w, rw, wb, "weights")
    ray_b = wb[:, -1:]  # >= every weight's bound of the ray
    check(acc, ref["accumulation"], S * ray_b, "accumulation")
    mid = ((s + e) / np.float32(2)).astype(np.float64)
    check(depth, ref["depth"], S * ray_b * np.abs(mid).max(-1, keepdims=True), "depth")
    rfeat = ref["feature"].reshape(Rr, S, -1).astype(np.float64)
    fmax = np.abs(rfeat).max(1)
    # features: the weight errors times the feature size, the sky residual's error on the last sample, and the field's own
    # fp32 feature error (1e-5 of its size) under weights that sum to at most 1
    check(feats, ref["features"], 2 * S * ray_b * fmax + 1e-5 * (1 + fmax), "features")
    # the per-sample features themselves
    check(host64(f2).reshape(Rr, S, -1), rfeat, 1e-5 * (1 + np.abs(rfeat)), "per-sample features")
