"""Packed (ragged) compositing of the occupancy-marched samples, forward and backward, from the kernels to the renderers.
What is pinned: the reference's RaySamples.get_weights golden on truncated rays (1), a float64 restatement written from
the formulas (tests/packed_restatement.py) for every op's forward and -- through float64 torch autograd -- backward (2, 3),
the dense kernels on uniform segments (4), the saturated input families of tests/sharp_refs.py per element (5),
bitwise reproducibility (6), the segment search (7), the module-level sequence VolumetricSampler -> field -> packed
renderers (8), the dense operator path end to end (9) and graph capture (10).  Parity with nerfacc itself stays unpinned.
Tolerances are those of tests/test_gpu_parity.py for the dense kernels this mirrors."""
import numpy as np
import pytest
import torch

import packed_restatement as PR
import synth
from conftest import load_golden, rel_l2
from gpu_util import cuda, host64, make_field, ray_bundle
from gpu_util import ops  # noqa: F401  (fixture)
from sharp_refs import SAMPLES, TINY, U, check, ref_alpha, ref_density, sharp_alphas, sharp_bins

pytestmark = pytest.mark.gpu

TIGHT, TOL = 2e-5, 1e-4
CHANNELS = [1, 3, 32, 48]


def ragged_counts(R, seed):
    """segment lengths: the chunk edges of a 64-lane walk, long rays, random ones, and empty rays at the front, in the
    middle (two in a row) and at the end"""
    rng = np.random.default_rng(seed)
    special = np.array([0, 1, 2, 63, 64, 65, 130, 300])
    c = np.where(rng.random(R) < 0.5, rng.choice(special, R), rng.integers(0, 200, R))
    c[1:1 + len(special)] = special
    c[0] = c[R // 2] = c[R // 2 + 1] = c[-1] = 0
    return c.astype(np.int64)


def ragged_inputs(seed, C, R=200):
    counts = ragged_counts(R, seed)
    seg = PR.segments_from_counts(counts)
    M = int(seg[-1])
    width = synth.uniform((M,), 0.01, 0.5, seed + 1)
    gap = synth.uniform((M,), 0.0, 0.2, seed + 2)
    ts, te = np.empty(M, np.float32), np.empty(M, np.float32)
    for r in range(R):  # sorted, non-overlapping intervals along each ray
        b, e = seg[r], seg[r + 1]
        edge = np.cumsum(width[b:e] + gap[b:e]) + np.float32(0.5)
        te[b:e] = edge
        ts[b:e] = edge - width[b:e]
    sig = np.exp(synth.uniform((M,), -5.0, 1.5, seed + 3)).astype(np.float32)
    alpha = synth.uniform((M,), 0.0, 1.0, seed + 4) ** 3
    alpha = np.where(synth.uniform((M,), 0, 1, seed + 5) < 0.1, np.float32(0.0), alpha).astype(np.float32)
    feat = synth.normal((M, C), seed + 6)
    return dict(counts=counts, seg=seg, M=M, R=R, ts=ts, te=te, sig=sig, alpha=alpha, feat=feat)


def on_device(p):
    return {k: (cuda(v) if isinstance(v, np.ndarray) and k != "counts" else v) for k, v in p.items()}


# ---- 1. reference anchor ---------------------------------------------------------------------------------------------
def test_packed_weights_against_the_reference_golden(ops):
    """RaySamples.get_weights of the reference (tests/golden/sampler_parts.npz).  A weight depends only on the samples in
    front of it, so the first n_r samples of ray r, packed, must reproduce w0[r, :n_r]."""
    g = load_golden("sampler_parts")
    eu, dens, w0 = g["eu0"], g["dens0"], g["w0"]
    R, S = dens.shape
    n = np.random.default_rng(7).integers(0, S + 1, R)
    n[[0, 5, 11, 17]] = [0, 1, 65, 128]
    seg = PR.segments_from_counts(n)
    pick = np.concatenate([np.arange(r * S, r * S + n[r]) for r in range(R)])
    ts, te = eu[:, :-1].reshape(-1)[pick], eu[:, 1:].reshape(-1)[pick]
    w, _, _ = ops.packed_weight_from_density(cuda(ts), cuda(te), cuda(dens.reshape(-1)[pick]), cuda(seg))
    want = w0.reshape(-1)[pick]
    ref = PR.weight_from_density(PR.f64(ts), PR.f64(te), PR.f64(dens.reshape(-1)[pick]), seg)[0].numpy()
    print(f"restatement vs golden {rel_l2(ref, want):.3g}, kernel vs golden {rel_l2(host64(w), want):.3g}")
    assert rel_l2(ref, want) < TIGHT
    assert rel_l2(host64(w), want) < TIGHT


# ---- 2. forward against the float64 restatement -------------------------------------------------------------------------
def test_weight_ops_forward(ops):
    p = ragged_inputs(11, 1)
    d = on_device(p)
    ts, te, sig, al = (PR.f64(p[k]) for k in ("ts", "te", "sig", "alpha"))
    w, t, a = ops.packed_weight_from_density(d["ts"], d["te"], d["sig"], d["seg"])
    rw, rt, ra = PR.weight_from_density(ts, te, sig, p["seg"])
    for got, want, what in ((w, rw, "weights"), (t, rt, "trans"), (a, ra, "alphas")):
        err = rel_l2(host64(got), want.numpy())
        print(f"density {what}: {err:.3g}")
        assert np.isfinite(host64(got)).all() and err < TIGHT, what
    w, t = ops.packed_weight_from_alpha(d["alpha"], d["seg"])
    rw, rt = PR.weight_from_alpha(al, p["seg"])
    for got, want, what in ((w, rw, "weights"), (t, rt, "trans")):
        err = rel_l2(host64(got), want.numpy())
        print(f"alpha {what}: {err:.3g}")
        assert np.isfinite(host64(got)).all() and err < TIGHT, what


@pytest.mark.parametrize("C", CHANNELS)
def test_accumulate_and_composite_forward(ops, C):
    p = ragged_inputs(20 + C, C)
    d = on_device(p)
    empty = p["counts"] == 0
    ts, te, sig, al, feat = (PR.f64(p[k]) for k in ("ts", "te", "sig", "alpha", "feat"))
    w64 = PR.weight_from_alpha(al, p["seg"])[0]
    w32 = cuda(w64.numpy().astype(np.float32))
    out = ops.packed_accumulate(w32, d["feat"], d["seg"])
    want = PR.accumulate(PR.f64(w32), feat, p["seg"]).numpy()
    assert out.shape == (p["R"], C) and rel_l2(host64(out), want) < TIGHT
    assert (host64(out)[empty] == 0).all() and np.isfinite(host64(out)).all()
    out1 = ops.packed_accumulate(w32, None, d["seg"])
    assert out1.shape == (p["R"], 1) and rel_l2(host64(out1), PR.accumulate(PR.f64(w32), None, p["seg"]).numpy()) < TIGHT
    assert (host64(out1)[empty] == 0).all()
    for density_mode, x64, x in ((True, sig, d["sig"]), (False, al, d["alpha"])):
        of, od, oa, ow = ops.packed_composite_fwd(d["ts"], d["te"], x, d["feat"], d["seg"], density_mode)
        rf, rd, ra, rw = PR.composite(ts, te, x64, feat, p["seg"], density_mode)
        for got, want, what in ((of, rf, "features"), (od, rd, "depth"), (oa, ra, "accumulation"), (ow, rw, "weights")):
            err = rel_l2(host64(got), want.numpy())
            print(f"C={C} density_mode={density_mode} {what}: {err:.3g}")
            assert got.shape == want.shape and np.isfinite(host64(got)).all() and err < TIGHT, (what, density_mode)
        for got in (of, od, oa):
            assert (host64(got)[empty] == 0).all()
        # the unfused chain gives the same numbers as the fused kernel
        w_unf = (ops.packed_weight_from_density(d["ts"], d["te"], x, d["seg"]) if density_mode
                 else ops.packed_weight_from_alpha(x, d["seg"]))[0]
        assert torch.equal(w_unf, ow)
        assert ops.packed_composite_fwd(d["ts"], d["te"], x, d["feat"], d["seg"], density_mode, return_weights=False)[3] is None


@pytest.mark.parametrize("C", CHANNELS)
def test_no_samples_gives_zero_rows(ops, C):
    R = 9
    seg = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    e = torch.empty(0, device="cuda")
    ef = torch.empty((0, C), device="cuda")
    out = ops.packed_accumulate(e, ef, seg)
    assert out.shape == (R, C) and (out == 0).all()
    assert (ops.packed_accumulate(e, None, seg) == 0).all()
    for mode in (True, False):
        of, od, oa, ow = ops.packed_composite_fwd(e, e, e, ef, seg, mode)
        assert of.shape == (R, C) and od.shape == (R, 1) and oa.shape == (R, 1) and ow.shape == (0,)
        assert (of == 0).all() and (od == 0).all() and (oa == 0).all()
        gx, gf = ops.packed_composite_bwd(e, e, e, ef, seg, mode, torch.ones((R, C), device="cuda"))
        assert gx.shape == (0,) and gf.shape == (0, C)
    assert ops.packed_weight_from_alpha(e, seg)[0].shape == (0,)
    assert torch.equal(ops.packed_segments(torch.empty(0, dtype=torch.int64, device="cuda"), R), seg)


# ---- 3. backward against float64 autograd of the restatement -----------------------------------------------------------
def test_weight_ops_backward(ops):
    p = ragged_inputs(31, 1)
    d = on_device(p)
    M = p["M"]
    gw, gt = synth.normal((M,), 32), synth.normal((M,), 33)
    sig = PR.f64(p["sig"], grad=True)
    (PR.weight_from_density(PR.f64(p["ts"]), PR.f64(p["te"]), sig, p["seg"])[0] * PR.f64(gw)).sum().backward()
    gs = ops.packed_weight_from_density_bwd(d["ts"], d["te"], d["sig"], d["seg"], cuda(gw))
    err = rel_l2(host64(gs), sig.grad.numpy())
    print(f"grad_sigmas: {err:.3g}")
    assert np.isfinite(host64(gs)).all() and err < TOL
    for with_gt in (True, False):
        al = PR.f64(p["alpha"], grad=True)
        w, t = PR.weight_from_alpha(al, p["seg"])
        ((w * PR.f64(gw)).sum() + ((t * PR.f64(gt)).sum() if with_gt else 0)).backward()
        ga = ops.packed_weight_from_alpha_bwd(d["alpha"], d["seg"], cuda(gw), cuda(gt) if with_gt else None)
        err = rel_l2(host64(ga), al.grad.numpy())
        print(f"grad_alphas (grad_t {with_gt}): {err:.3g}")
        assert np.isfinite(host64(ga)).all() and err < TOL


def test_weight_autograd_nodes(ops):
    """the autograd nodes: density mode differentiates the weights only, alpha mode the weights and the transmittance"""
    from neurad_studio_amd import autograd as ag

    p = ragged_inputs(35, 1)
    d = on_device(p)
    gw, gt = cuda(synth.normal((p["M"],), 36)), cuda(synth.normal((p["M"],), 37))
    sig = d["sig"].clone().requires_grad_(True)
    w, t, a = ag.PackedWeightFromDensityFn.apply(d["ts"], d["te"], sig, d["seg"])
    assert w.requires_grad and not t.requires_grad and not a.requires_grad
    (w * gw).sum().backward()
    assert torch.equal(sig.grad, ops.packed_weight_from_density_bwd(d["ts"], d["te"], d["sig"], d["seg"], gw))
    al = d["alpha"].clone().requires_grad_(True)
    w, t = ag.PackedWeightFromAlphaFn.apply(al, d["seg"])
    ((w * gw).sum() + (t * gt).sum()).backward()
    assert torch.equal(al.grad, ops.packed_weight_from_alpha_bwd(d["alpha"], d["seg"], gw, gt))


@pytest.mark.parametrize("C", CHANNELS)
def test_accumulate_backward(ops, C):
    from neurad_studio_amd import autograd as ag

    p = ragged_inputs(40 + C, C)
    d = on_device(p)
    w32 = synth.uniform((p["M"],), 0.0, 1.0, 41)
    g = synth.normal((p["R"], C), 42)
    w, v = PR.f64(w32, grad=True), PR.f64(p["feat"], grad=True)
    (PR.accumulate(w, v, p["seg"]) * PR.f64(g)).sum().backward()
    gw, gv = ops.packed_accumulate_bwd(cuda(w32), d["feat"], cuda(g), d["seg"])
    print(f"C={C} grad_weights {rel_l2(host64(gw), w.grad.numpy()):.3g} grad_values {rel_l2(host64(gv), v.grad.numpy()):.3g}")
    assert rel_l2(host64(gw), w.grad.numpy()) < TIGHT and rel_l2(host64(gv), v.grad.numpy()) < TIGHT
    # each gradient only when it is needed
    only_w = ops.packed_accumulate_bwd(cuda(w32), d["feat"], cuda(g), d["seg"], need_grad_values=False)
    only_v = ops.packed_accumulate_bwd(cuda(w32), d["feat"], cuda(g), d["seg"], need_grad_weights=False)
    assert only_w[1] is None and torch.equal(only_w[0], gw) and only_v[0] is None and torch.equal(only_v[1], gv)
    wt, vt = cuda(w32).requires_grad_(True), d["feat"].clone().requires_grad_(True)
    (ag.PackedAccumulateFn.apply(wt, vt.detach(), d["seg"]) * cuda(g)).sum().backward()
    assert torch.equal(wt.grad, gw) and vt.grad is None
    (ag.PackedAccumulateFn.apply(wt.detach(), vt, d["seg"]) * cuda(g)).sum().backward()
    assert torch.equal(vt.grad, gv)
    # without values: the plain sum
    g1 = synth.normal((p["R"], 1), 43)
    w1 = PR.f64(w32, grad=True)
    (PR.accumulate(w1, None, p["seg"]) * PR.f64(g1)).sum().backward()
    wt = cuda(w32).requires_grad_(True)
    (ag.PackedAccumulateFn.apply(wt, None, d["seg"]) * cuda(g1)).sum().backward()
    assert rel_l2(host64(wt.grad), w1.grad.numpy()) < TIGHT


@pytest.mark.parametrize("density_mode", [True, False], ids=["density", "alpha"])
@pytest.mark.parametrize("C", CHANNELS)
def test_composite_backward(ops, C, density_mode):
    """the fused node against float64 autograd of the restatement, and against the three unfused nodes chained"""
    from neurad_studio_amd import autograd as ag

    p = ragged_inputs(50 + C, C)
    d = on_device(p)
    R, M = p["R"], p["M"]
    gF, gD, gA, gW = synth.normal((R, C), 51), synth.normal((R, 1), 52), synth.normal((R, 1), 53), synth.normal((M,), 54)
    key = "sig" if density_mode else "alpha"
    x64, f64 = PR.f64(p[key], grad=True), PR.f64(p["feat"], grad=True)
    rf, rd, ra, rw = PR.composite(PR.f64(p["ts"]), PR.f64(p["te"]), x64, f64, p["seg"], density_mode)
    ((rf * PR.f64(gF)).sum() + (rd * PR.f64(gD)).sum() + (ra * PR.f64(gA)).sum() + (rw * PR.f64(gW)).sum()).backward()

    def run(fused):
        x, f = d[key].clone().requires_grad_(True), d["feat"].clone().requires_grad_(True)
        if fused:
            of, od, oa, ow = ag.PackedCompositeFn.apply(d["ts"], d["te"], x, f, d["seg"], density_mode)
        else:
            ow = (ag.PackedWeightFromDensityFn.apply(d["ts"], d["te"], x, d["seg"]) if density_mode
                  else ag.PackedWeightFromAlphaFn.apply(x, d["seg"]))[0]
            of = ag.PackedAccumulateFn.apply(ow, f, d["seg"])
            od = ag.PackedAccumulateFn.apply(ow, ((d["ts"] + d["te"]) / 2)[:, None], d["seg"])
            oa = ag.PackedAccumulateFn.apply(ow, None, d["seg"])
        ((of * cuda(gF)).sum() + (od * cuda(gD)).sum() + (oa * cuda(gA)).sum() + (ow * cuda(gW)).sum()).backward()
        return x.grad, f.grad

    gx, gf = run(True)
    ux, uf = run(False)
    e_x, e_f = rel_l2(host64(gx), x64.grad.numpy()), rel_l2(host64(gf), f64.grad.numpy())
    e_ux, e_uf = rel_l2(host64(gx), host64(ux)), rel_l2(host64(gf), host64(uf))
    print(f"C={C} {key}: grad_x {e_x:.3g} grad_features {e_f:.3g}; fused vs unfused {e_ux:.3g} {e_uf:.3g}")
    assert np.isfinite(host64(gx)).all() and np.isfinite(host64(gf)).all()
    assert e_x < TOL and e_f < TIGHT
    assert e_ux < TIGHT and e_uf < TIGHT
    # only the outputs that were used send a gradient; only the inputs that need one get it
    x = d[key].clone().requires_grad_(True)
    of = ag.PackedCompositeFn.apply(d["ts"], d["te"], x, d["feat"], d["seg"], density_mode)[0]
    (of * cuda(gF)).sum().backward()
    want, none = ops.packed_composite_bwd(d["ts"], d["te"], d[key], d["feat"], d["seg"], density_mode, cuda(gF),
                                          need_grad_features=False)
    assert none is None and torch.equal(x.grad, want)


# ---- 4. dense equivalence ------------------------------------------------------------------------------------------------
def test_uniform_segments_agree_with_the_dense_kernels(ops):
    from neurad_studio_amd import autograd as ag
    from neurad_studio_amd.shims import nerfacc

    R, S, C = 37, 70, 32
    e = np.cumsum(synth.uniform((R, S + 1), 0.01, 0.4, 60), -1).astype(np.float32)
    ts, te = cuda(e[:, :-1]), cuda(e[:, 1:])
    sig = cuda(np.exp(synth.uniform((R, S), -5.0, 1.5, 61)))
    al = cuda(synth.uniform((R, S), 0.0, 1.0, 62) ** 3)
    feat = cuda(synth.normal((R, S, C), 63))
    before = nerfacc.render_weight_from_density(ts, te, sig), nerfacc.render_weight_from_alpha(al)
    seg = torch.arange(R + 1, device="cuda") * S
    pw, pt, pa = ops.packed_weight_from_density(ts, te, sig, seg)
    dw, dt, da = ops.render_weight_from_density(ts, te, sig)
    for got, want, what in ((pw, dw, "w"), (pt, dt, "T"), (pa, da, "alpha")):
        assert rel_l2(host64(got), host64(want).reshape(-1)) < 2 * TIGHT, what
    pw, pt = ops.packed_weight_from_alpha(al, seg)
    dw, dt = ops.render_weight_from_alpha(al)
    assert rel_l2(host64(pw), host64(dw).reshape(-1)) < 2 * TIGHT and rel_l2(host64(pt), host64(dt).reshape(-1)) < 2 * TIGHT
    assert rel_l2(host64(ops.packed_accumulate(dw, feat.reshape(-1, C), seg)), host64(ops.accumulate_along_rays(dw, feat))) < 2 * TIGHT
    assert rel_l2(host64(ops.packed_accumulate(dw, None, seg)), host64(ops.accumulate_along_rays(dw))) < 2 * TIGHT
    # the packed call through the shim is the same kernel
    ri = torch.arange(R, device="cuda").repeat_interleave(S)
    assert torch.equal(nerfacc.render_weight_from_alpha(al.reshape(-1), ray_indices=ri, n_rays=R)[0], pw)
    assert torch.equal(nerfacc.render_weight_from_alpha(al.reshape(-1), packed_info=nerfacc.pack_info(ri, R))[0], pw)
    # the dense branches are what they were: the same nodes, the same tensors, before and after packed calls
    after = nerfacc.render_weight_from_density(ts, te, sig), nerfacc.render_weight_from_alpha(al)
    direct = ag.WeightFromDensityFn.apply(ts, te, sig), ag.WeightFromAlphaFn.apply(al)
    for b, a, c in zip(before, after, direct):
        for x, y, z in zip(b, a, c):
            assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(nerfacc.accumulate_along_rays(dw, feat), ag.AccumulateFn.apply(dw, feat))
    assert torch.equal(nerfacc.accumulate_along_rays(dw), ops.accumulate_along_rays(dw))


# ---- 5. saturation -------------------------------------------------------------------------------------------------------
def packed_blocks(blocks):
    """dense [R,S] blocks of different S -> one ragged batch with an empty ray between the blocks; -> seg, and a function
    that packs a list of per-block arrays (trailing dims kept) the same way"""
    counts = []
    for b in blocks:
        counts += [b.shape[1]] * b.shape[0] + [0]
    return PR.segments_from_counts(counts), lambda arrs: np.concatenate([a.reshape((-1,) + a.shape[2:]) for a in arrs])


def test_alpha_mode_saturated(ops):
    blocks = [sharp_alphas(S, 10 + S) for S in SAMPLES]
    seg, pack = packed_blocks(blocks)
    gws = [synth.normal(b.shape, 20 + b.shape[1]) for b in blocks]
    gts = [synth.normal(b.shape, 30 + b.shape[1]) for b in blocks]
    a = pack(blocks)
    w, t = ops.packed_weight_from_alpha(cuda(a), cuda(seg))
    ga = host64(ops.packed_weight_from_alpha_bwd(cuda(a), cuda(seg), cuda(pack(gws)), cuda(pack(gts))))
    ga0 = host64(ops.packed_weight_from_alpha_bwd(cuda(a), cuda(seg), cuda(pack(gws))))
    refs = [ref_alpha(b, gw, gt) for b, gw, gt in zip(blocks, gws, gts)]
    refs0 = [ref_alpha(b, gw, np.zeros_like(gt)) for b, gw, gt in zip(blocks, gws, gts)]
    rtol = pack([np.full(b.shape, 2 * (b.shape[1] + 2) * U) for b in blocks])
    gtol = pack([np.full(b.shape, 4 * (b.shape[1] + 8) * U) for b in blocks])
    gscale = pack([np.broadcast_to(np.abs(gw).max(-1, keepdims=True) + np.abs(gt).max(-1, keepdims=True), gw.shape)
                   for gw, gt in zip(gws, gts)])
    rw, rt, rga, mag = (pack([r[k] for r in refs]) for k in range(4))
    check(host64(w), rw, TINY + rtol * rw, "weights")
    check(host64(t), rt, TINY + rtol * rt, "trans")
    assert (host64(w)[a == 0] == 0).all()
    check(ga, rga, 2.0 ** -100 * gscale + gtol * mag, "dL/dalpha")
    check(ga0, pack([r[2] for r in refs0]), 2.0 ** -100 * gscale + gtol * pack([r[3] for r in refs0]), "dL/dalpha (no grad_t)")


def test_density_mode_saturated(ops):
    bins = [sharp_bins(S, 40 + S) for S in SAMPLES]
    seg, pack = packed_blocks([b[2] for b in bins])
    gws = [synth.normal(b[2].shape, 50 + b[2].shape[1]) for b in bins]
    st, en, sig = (pack([b[k] for b in bins]) for k in range(3))
    refs = [ref_density(b[1] - b[0], b[2], gw) for b, gw in zip(bins, gws)]
    rw, rt, ra, rgs, fscale, gscale = (pack([r[k] for r in refs]) for k in range(6))
    w, t, a = ops.packed_weight_from_density(cuda(st), cuda(en), cuda(sig), cuda(seg))
    check(host64(w), rw, TINY + fscale, "weights")
    check(host64(t), rt, TINY + fscale, "trans")
    check(host64(a), ra, TINY + 4 * U, "alphas")
    gs = host64(ops.packed_weight_from_density_bwd(cuda(st), cuda(en), cuda(sig), cuda(seg), cuda(pack(gws))))
    atol = pack([TINY * ((b[1] - b[0]).astype(np.float64) + 1) * np.abs(gw).max(-1, keepdims=True) for b, gw in zip(bins, gws)])
    check(gs, rgs, atol + gscale, "dL/dsigma")


@pytest.mark.parametrize("C", [32, 3])
def test_fused_composite_saturated(ops, C):
    """The fused node on the same families.  The gradient that reaches a weight is G_i = gW_i + gA + gD mid_i + sum_c gF_c
    f_ic; the weight backward is then held to the dense bounds with gw := G (float64) -- alpha mode as
    test_sdf_render_saturated does (4 (S + C + 8) u of the magnitude sum under |G|'s own magnitude sum), density mode as
    test_prop_weights_saturated does (gscale(G) + gscale(|G| terms)), the latter widened by (C + 4) / (4 (S + 4)): G's own
    C + 3 roundings enter the gradient through the very terms gscale adds up, each weighted 4 (S + 4) u there."""
    ablocks = [sharp_alphas(S, 110 + S) for S in SAMPLES]
    bins = [sharp_bins(S, 140 + S) for S in SAMPLES]
    for b in bins:  # (a sky edge of 1e10 would make the depth's midpoints the whole story)
        b[1][:, -1] = np.where(b[1][:, -1] > 1e9, np.maximum(np.float32(1e4), b[0][:, -1]), b[1][:, -1])
    seg, pack = packed_blocks(ablocks)
    R = len(seg) - 1
    rows = PR.ray_indices_from_segments(seg)
    gF, gD, gA = synth.normal((R, C), 150), synth.normal((R, 1), 151), synth.normal((R, 1), 152)
    feats = [synth.normal(b.shape + (C,), 160 + b.shape[1]) for b in ablocks]
    gWs = [synth.normal(b.shape, 170 + b.shape[1]) for b in ablocks]
    st, en, sig, al, feat, gW = (pack(v) for v in ([b[0] for b in bins], [b[1] for b in bins], [b[2] for b in bins],
                                                   ablocks, feats, gWs))
    mid = ((st + en) / np.float32(2)).astype(np.float64)
    q = (feat.astype(np.float64) * gF[rows].astype(np.float64)).sum(-1)
    qm = (np.abs(feat.astype(np.float64)) * np.abs(gF[rows]).astype(np.float64)).sum(-1)
    G = gW + gA[rows, 0].astype(np.float64) + gD[rows, 0] * mid + q
    Gm = np.abs(gW) + np.abs(gA[rows, 0]).astype(np.float64) + np.abs(gD[rows, 0] * mid) + qm
    unpack = lambda v: np.split(v, np.cumsum([b.size for b in ablocks])[:-1])  # noqa: E731
    Gb = [g.reshape(b.shape) for g, b in zip(unpack(G), ablocks)]
    Gmb = [g.reshape(b.shape) for g, b in zip(unpack(Gm), ablocks)]
    d = dict(ts=cuda(st), te=cuda(en), seg=cuda(seg), feat=cuda(feat))
    for density_mode, x in ((False, al), (True, sig)):
        of, od, oa, ow = ops.packed_composite_fwd(d["ts"], d["te"], cuda(x), d["feat"], d["seg"], density_mode)
        gx, gf = ops.packed_composite_bwd(d["ts"], d["te"], cuda(x), d["feat"], d["seg"], density_mode, cuda(gF), cuda(gD),
                                          cuda(gA), cuda(gW))
        for v in (of, od, oa, ow, gx, gf):
            assert torch.isfinite(v).all()
        w_unf = (ops.packed_weight_from_density(d["ts"], d["te"], cuda(x), d["seg"]) if density_mode
                 else ops.packed_weight_from_alpha(cuda(x), d["seg"]))[0]
        assert torch.equal(ow, w_unf)  # (held per element by the two tests above)
        w64 = host64(ow)
        rgf = w64[:, None] * gF[rows].astype(np.float64)
        check(host64(gf), rgf, TINY + 2 * U * np.abs(rgf), "d features")
        if density_mode:
            refs = [ref_density(b[1] - b[0], b[2], g) for b, g in zip(bins, Gb)]
            refs_m = [ref_density(b[1] - b[0], b[2], g) for b, g in zip(bins, Gmb)]
            widen = pack([np.full(b.shape, 1 + (C + 4) / (4 * (b.shape[1] + 4))) for b in ablocks])
            atol = pack([TINY * ((b[1] - b[0]).astype(np.float64) + 1) * g.max(-1, keepdims=True) for b, g in zip(bins, Gmb)])
            check(host64(gx), pack([r[3] for r in refs]), atol + pack([r[5] for r in refs]) + widen * pack([r[5] for r in refs_m]),
                  "dL/dsigma")
        else:
            refs = [ref_alpha(b, g, np.zeros_like(g)) for b, g in zip(ablocks, Gb)]
            refs_m = [ref_alpha(b, g, np.zeros_like(g)) for b, g in zip(ablocks, Gmb)]
            gtol = pack([np.full(b.shape, 4 * (b.shape[1] + C + 8) * U) for b in ablocks])
            gscale = pack([np.broadcast_to(g.max(-1, keepdims=True), g.shape) for g in Gmb])
            check(host64(gx), pack([r[2] for r in refs]), 2.0 ** -100 * gscale + gtol * pack([r[3] for r in refs_m]), "dL/dalpha")


# ---- 6. reproducibility --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 3])
def test_fused_forward_and_backward_are_bitwise_reproducible(ops, C):
    p = ragged_inputs(70 + C, C)
    d = on_device(p)
    gF, gD, gA = cuda(synth.normal((p["R"], C), 71)), cuda(synth.normal((p["R"], 1), 72)), cuda(synth.normal((p["R"], 1), 73))
    for mode, key in ((True, "sig"), (False, "alpha")):
        runs = []
        for _ in range(2):
            fwd = ops.packed_composite_fwd(d["ts"], d["te"], d[key], d["feat"], d["seg"], mode)
            bwd = ops.packed_composite_bwd(d["ts"], d["te"], d[key], d["feat"], d["seg"], mode, gF, gD, gA)
            runs.append(fwd + bwd)
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ---- 7. segments -----------------------------------------------------------------------------------------------------------
def test_packed_segments_and_pack_info(ops):
    from neurad_studio_amd.shims import nerfacc

    cases = [ragged_counts(200, 80), np.array([0, 0, 3, 0, 0, 5, 1, 0, 0]), np.array([4]), np.array([0]), np.zeros(7, np.int64),
             np.full(1000, 3)]
    for counts in cases:
        R = len(counts)
        seg = PR.segments_from_counts(counts)
        ri = cuda(PR.ray_indices_from_segments(seg))
        got = ops.packed_segments(ri, R)
        want = torch.searchsorted(ri, torch.arange(R + 1, device="cuda"))
        assert got.dtype == torch.int64 and torch.equal(got, want) and torch.equal(got, cuda(seg))
        info = nerfacc.pack_info(ri, R)
        assert info.shape == (R, 2) and torch.equal(info[:, 1], cuda(np.asarray(counts, np.int64)))
        assert torch.equal(info[:, 0], cuda(seg[:-1]))
        if ri.numel():
            assert torch.equal(torch.repeat_interleave(torch.arange(R, device="cuda"), info[:, 1]), ri)


# ---- 8. module level -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_volumetric_sampler_field_packed_renderers(ops, use_sdf):
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.model_components.renderers import (AccumulationRenderer, DepthRenderer, FeatureRenderer,
                                                              NormalsRenderer, render_depth_simple, render_packed)
    from neurad_studio_amd.shims import nerfacc
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    R = 96
    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    est.binaries[0] = cuda(np.random.default_rng(3).random((16, 16, 16)) < 0.3)
    rb = ray_bundle(R, 90, far=9.0)
    rs, ri = VolumetricSampler(est).eval()(rb, render_step_size=0.2, cone_angle=0.05)
    M = ri.shape[0]
    counts = torch.bincount(ri, minlength=R).cpu().numpy()
    assert M > 4 * R and (counts == 0).any() and counts.max() > 8 and rs.frustums.starts.shape == (M, 1)
    seg = PR.segments_from_counts(counts)
    fld = make_field(use_sdf).eval()
    with torch.no_grad():
        out = fld(rs)
    feat = out[FieldHeadNames.FEATURE]
    assert feat.shape == (M, fld.config.nff_out_dim)
    ts, te = PR.f64(rs.frustums.starts[:, 0]), PR.f64(rs.frustums.ends[:, 0])
    if use_sdf:
        head = out[FieldHeadNames.ALPHA]
        weights = nerfacc.render_weight_from_alpha(head[..., 0], ray_indices=ri, n_rays=R)[0][..., None]
        w64 = PR.weight_from_alpha(PR.f64(head[:, 0]), seg)[0]
    else:
        head = out[FieldHeadNames.DENSITY]
        weights = nerfacc.render_weight_from_density(rs.frustums.starts[..., 0], rs.frustums.ends[..., 0], head[..., 0],
                                                     ray_indices=ri, n_rays=R)[0][..., None]
        w64 = PR.weight_from_density(ts, te, PR.f64(head[:, 0]), seg)[0]
    assert head.shape == (M, 1) and weights.shape == (M, 1)
    mid = ((rs.frustums.starts + rs.frustums.ends) / 2)
    normals = torch.nn.functional.normalize(feat[:, :3], dim=-1)
    want_f = PR.accumulate(w64, PR.f64(feat), seg).numpy()
    want_a = PR.accumulate(w64, None, seg).numpy()
    want_d = PR.accumulate(w64, PR.f64(mid), seg).numpy()
    want_n = PR.accumulate(w64, PR.f64(normals), seg).numpy()
    assert rel_l2(host64(weights[:, 0]), w64.numpy()) < TIGHT
    assert rel_l2(host64(FeatureRenderer()(feat, weights, ray_indices=ri, num_rays=R)), want_f) < TIGHT
    assert rel_l2(host64(AccumulationRenderer()(weights, ray_indices=ri, num_rays=R)), want_a) < TIGHT
    assert rel_l2(host64(render_depth_simple(weights, rs, ray_indices=ri, num_rays=R)), want_d) < TIGHT
    assert rel_l2(host64(NormalsRenderer()(normals, weights, normalize=False, ray_indices=ri, num_rays=R)), want_n) < TIGHT
    n_norm = want_n / (np.linalg.norm(want_n, axis=-1, keepdims=True) + 1e-10)
    assert rel_l2(host64(NormalsRenderer()(normals, weights, ray_indices=ri, num_rays=R)), n_norm) < TIGHT
    want_depth = np.clip(want_d / (want_a + 1e-10), float(mid.min()), float(mid.max()))
    got_depth = DepthRenderer()(weights, rs, ray_indices=ri, num_rays=R)
    assert got_depth.shape == (R, 1) and rel_l2(host64(got_depth), want_depth) < TIGHT
    kw = {"alpha": head} if use_sdf else {"density": head}
    fused = render_packed(feat, rs, ri, R, **kw)
    assert fused["weights"].shape == (M, 1)
    for key, want in (("features", want_f), ("depth", want_d), ("accumulation", want_a), ("weights", w64.numpy()[:, None])):
        assert rel_l2(host64(fused[key]), want) < TIGHT, key
    # training: the loss reaches the hash table and the MLPs through the fused node
    fld.train()
    out = fld(rs)
    head = out[FieldHeadNames.ALPHA if use_sdf else FieldHeadNames.DENSITY]
    fused = render_packed(out[FieldHeadNames.FEATURE], rs, ri, R, **({"alpha": head} if use_sdf else {"density": head}))
    loss = (fused["features"] ** 2).mean() + fused["depth"].mean() + (fused["accumulation"] ** 2).mean()
    loss.backward()
    grads = [fld.hashgrid.static_grid.hash_table.grad] + [l.weight.grad for l in fld.mlp_geo.layers] + \
        [l.weight.grad for l in fld.mlp_feature.layers]
    for g in grads:
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0


# ---- 9. end to end against the dense path -----------------------------------------------------------------------------
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_packed_path_agrees_with_the_dense_operator_path(ops, use_sdf):
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.model_components.renderers import render_packed
    from neurad_studio_amd.shims import nerfacc
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    R, S = 32, 12
    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    from neurad_studio_amd.cameras.rays import RayBundle

    d = synth.normal((R, 3), 6)
    rb = RayBundle(origins=torch.zeros(R, 3, device="cuda"),
                   directions=cuda((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)),
                   pixel_area=torch.full((R, 1), 1e-6, device="cuda"), nears=torch.zeros(R, 1, device="cuda"),
                   fars=torch.full((R, 1), 3.0, device="cuda"))
    rs, ri = VolumetricSampler(est).eval()(rb, render_step_size=0.25)
    assert ri.shape[0] == R * S and torch.equal(ri, torch.arange(R, device="cuda").repeat_interleave(S))
    fld = make_field(use_sdf).eval()
    key = FieldHeadNames.ALPHA if use_sdf else FieldHeadNames.DENSITY
    starts, ends = rs.frustums.starts.reshape(R, S, 1), rs.frustums.ends.reshape(R, S, 1)
    dense = RaySamples(frustums=Frustums(origins=rb.origins[:, None].expand(R, S, 3), directions=rb.directions[:, None].expand(R, S, 3),
                                         starts=starts, ends=ends, pixel_area=rb.pixel_area[:, None].expand(R, S, 1)))
    with torch.no_grad():
        out_d, out_p = fld(dense), fld(rs)
    if use_sdf:
        w = nerfacc.render_weight_from_alpha(out_d[key][..., 0])[0]
    else:
        w = nerfacc.render_weight_from_density(starts[..., 0], ends[..., 0], out_d[key][..., 0])[0]
    feats = nerfacc.accumulate_along_rays(w, out_d[FieldHeadNames.FEATURE])
    acc = nerfacc.accumulate_along_rays(w)
    depth = nerfacc.accumulate_along_rays(w, (starts + ends) / 2)
    fused = render_packed(out_p[FieldHeadNames.FEATURE], rs, ri, R, **({"alpha": out_p[key]} if use_sdf else {"density": out_p[key]}))
    for name, got, want in (("features", fused["features"], feats), ("accumulation", fused["accumulation"], acc),
                            ("depth", fused["depth"], depth)):
        err = rel_l2(host64(got), host64(want))
        print(f"{name}: packed vs dense {err:.3g}")
        assert err < TOL, name


# ---- 10. graph capture -----------------------------------------------------------------------------------------------------
def test_fused_forward_and_backward_replay_in_a_graph(ops):
    C = 32
    p = ragged_inputs(95, C)
    d = on_device(p)
    gF, gD, gA = cuda(synth.normal((p["R"], C), 96)), cuda(synth.normal((p["R"], 1), 97)), cuda(synth.normal((p["R"], 1), 98))

    def step():
        fwd = ops.packed_composite_fwd(d["ts"], d["te"], d["sig"], d["feat"], d["seg"], True)
        return fwd + ops.packed_composite_bwd(d["ts"], d["te"], d["sig"], d["feat"], d["seg"], True, gF, gD, gA)

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    d["sig"].mul_(0.5)  # new values in the same buffers: the replay computes them
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(step(), captured):
        assert torch.equal(a, b)
