"""The sampler kernels (csrc/sampler.hip) at a trained scene's numerics, element by element against the float64 references of
tests/sampler_refs.py: PDF resampling inside its bracket, euclidean bins inside the propagated bound of the power transform,
the fused proposal sampler stage by stage -- each stage against the kernel's OWN previous outputs, so that the
discontinuous stage cannot blame its input.  A failing check names its first offending element with got, bound and the worst
err / bound in the assertion message; a passing test prints its worst err / bound (visible with -s)."""
import numpy as np
import pytest
import torch

import neurad_oracle as O
import sampler_refs as SR
import synth
from builders import trajectories
from gpu_util import actor_rays, cuda, dev, host, to_pspec
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
SKY = 20000.0


def _opt(a):
    return None if a is None else dev(a)


# ---- A. ops.pdf_sample ---------------------------------------------------------------------------------------------------
def _run_pdf(ops, c):
    sp, eu = ops.pdf_sample(dev(c["w"]), dev(c["bins"]), _opt(c["nears"]), dev(c["fars"]), c["Sn"], c["lam"], c["scaling"],
                            c["pad"], rand=_opt(c["rand"]))
    return host(sp), host(eu)


def _check_pdf(c, sp, eu):
    used, _ = SR.check_case_bins(c, sp)
    return used, SR.check_euclid(eu, sp, c["nears"], c["fars"], c["name"], c["lam"], c["scaling"])


@pytest.mark.parametrize("counts", SR.COUNTS, ids=[f"{a}-{b}" for a, b in SR.COUNTS])
def test_pdf_sample_inside_the_bracket(ops, counts):
    worst = [0.0, 0.0]
    for c in SR.cases(counts):
        worst = np.maximum(worst, _check_pdf(c, *_run_pdf(ops, c)))
    print(f"pdf_sample {counts}: share of DELTA used {worst[0]:.3g}, euclid err / bound width {worst[1]:.3g}")


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5])
def test_pdf_sample_workgroup_tail(ops, R):
    for rk in ("single", "perbin"):
        c = SR.make_case(65, 33, 0.01, rk, True, 20000.0, R=R)
        _check_pdf(c, *_run_pdf(ops, c))


def test_pdf_sample_strided_inputs(ops):
    c = SR.make_case(130, 65, 0.0, "perbin", True, 20000.0)
    w, bins, rand = dev(c["w"].T).t(), dev(c["bins"].T).t(), dev(c["rand"].T).t()
    nears = dev(np.stack([c["nears"], c["nears"] + 1], -1))[:, 0]
    fars = dev(np.stack([c["fars"], c["fars"] + 1], -1))[:, 0]
    assert not any(t.is_contiguous() for t in (w, bins, rand, nears, fars))
    sp, eu = ops.pdf_sample(w, bins, nears, fars, c["Sn"], c["lam"], c["scaling"], c["pad"], rand=rand)
    sp2, eu2 = _run_pdf(ops, c)
    assert np.array_equal(host(sp), sp2) and np.array_equal(host(eu), eu2)
    _check_pdf(c, host(sp), host(eu))


# ---- B. ops.power_sampler ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [-1.0, 0.0, 1.0, -2.0, 0.5])
def test_power_sampler_vs_oracle_with_near_planes(ops, lam):
    worst = 0.0
    for R in (13, 65):  # 65: one ray past the 64-ray workgroup
        nears = synth.uniform((R,), 0.5, 3.0, 5)
        fars = np.where(np.arange(R) % 3 == 0, 200.0, np.where(np.arange(R) % 3 == 1, SKY, 3.5)).astype(np.float32)
        for S in (1, 37, 64, 128):
            for t_rand in (None, synth.uniform((R, S + 1), 0.0, 1.0, 6 + S)):
                what = f"power_sampler lam={lam} R={R} S={S} jitter={t_rand is not None}"
                rsp, _, _ = O.power_sampler(nears, fars, S, lam, 0.1, t_rand)
                sp, eu = ops.power_sampler(dev(nears), dev(fars), S, lam, 0.1, _opt(t_rand))
                assert np.array_equal(host(sp), rsp), what  # spacing bins bit for bit
                worst = max(worst, SR.check_euclid(host(eu), host(sp), nears, fars, what, lam, 0.1))
    print(f"power_sampler lam={lam}: euclid err / bound width {worst:.3g}")


# ---- C. ops.proposal_sampler_fwd, stage by stage ---------------------------------------------------------------------------
def _fused(ops, monkeypatch, props, half, o, d, area, nears, fars, counts, pad, **actor_kw):
    """the fused launch with its outputs filled with NaN beforehand: an element no thread wrote stays NaN"""
    specs = props if actor_kw else [to_pspec(ops, p) for p in props]
    if half and not actor_kw:
        for s in specs:
            s.table = s.table.half()
    real = torch.empty
    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", lambda *a, **k: (lambda t: t.fill_(float("nan")) if t.is_floating_point() else t)(real(*a, **k)))
        ws, sps, eus = ops.proposal_sampler_fwd(specs, dev(o), dev(d), dev(area), _opt(nears), _opt(fars), counts,
                                                histogram_padding=pad, sky_distance=SKY, **actor_kw)
        torch.cuda.synchronize()
    return [host(w) for w in ws], [host(s) for s in sps], [host(e) for e in eus]


def _check_stages(ops, props, o, d, area, nears, fars, counts, pad, ws, sps, eus, what, stage2=True):
    """-> worst (stage 1 euclid, stage 2 weights, stage 3 DELTA share, stage 3 euclid) err / bound"""
    R = o.shape[0]
    far_used = np.minimum(np.full(R, SKY, np.float32) if fars is None else fars, np.float32(SKY))
    for a in (*ws, *sps, *eus):
        assert np.isfinite(a).all(), f"{what}: stale or non-finite output at rays {sorted(set(np.argwhere(~np.isfinite(a))[:, 0]))[:8]}"
    # stage 1: the round-0 bins are ops.power_sampler's, bit for bit (same expressions on the same inputs)
    sp0, eu0 = ops.power_sampler(_opt(nears), dev(far_used), counts[0])
    assert np.array_equal(sps[0], host(sp0)) and np.array_equal(eus[0], host(eu0)), f"{what}: stage 1 differs from power_sampler"
    out = [SR.check_euclid(eus[0], sps[0], nears, far_used, what + " stage 1"), 0.0, 0.0, 0.0]
    for k in range(len(counts) - 1):
        if stage2:  # stage 2: weights from the oracle's densities at the kernel's own edges
            dens = O.proposal_density(props[k], o, d, area, eus[k][:, :-1], eus[k][:, 1:])
            out[1] = max(out[1], SR.check_weights(ws[k], eus[k], dens, SR.prop_rho(props[k]), f"{what} round {k}"))
        # stage 3: new bins inside the bracket of the kernel's own weights and bins
        case = dict(w=ws[k], bins=sps[k], Sn=counts[k + 1], pad=pad, rand=None, name=f"{what} round {k}")
        out[2] = max(out[2], SR.check_case_bins(case, sps[k + 1])[0])
        out[3] = max(out[3], SR.check_euclid(eus[k + 1], sps[k + 1], nears, far_used, f"{what} round {k}"))
    return out


@pytest.mark.parametrize("v", SR.VARIANTS, ids=SR.VARIANT_IDS)
def test_fused_sampler_stage_by_stage(ops, monkeypatch, v):
    counts, levels, half, with_nears, fars_kind, pad, factor = v
    props = SR.variant_props(levels, half, factor)
    o, d, area, nears, fars = SR.variant_inputs(SR.R, with_nears, fars_kind)
    ws, sps, eus = _fused(ops, monkeypatch, props, half, o, d, area, nears, fars, counts, pad)
    if factor == SR.SHARP and levels[0] == 6 and not with_nears and fars_kind is None:
        assert 3 * (ws[0].max(-1) > 0.9).sum() >= SR.R  # a third of the rays with a bin of w > 0.9: a trained field
    r = _check_stages(ops, props, o, d, area, nears, fars, counts, pad, ws, sps, eus, "fused")
    print(f"fused {v}: euclid0 {r[0]:.3g}, weights {r[1]:.3g}, DELTA share {r[2]:.3g}, euclid {r[3]:.3g}")


@pytest.mark.parametrize("R", [1, 5, 33, 8192 + 37])
def test_fused_sampler_ray_distribution(ops, monkeypatch, R):
    """fewer than 8 workgroups (the XCD split at its smallest) and more than 2048 (the grid-stride wrap): every ray, every
    stage; nothing stale"""
    counts, pad = (16, 8, 4), 0.01
    props = SR.variant_props((6, 6), False, SR.SHARP)
    o, d, area, nears, fars = SR.variant_inputs(R, True, None)
    ws, sps, eus = _fused(ops, monkeypatch, props, False, o, d, area, nears, fars, counts, pad)
    for x in range(8):  # first and last ray of every XCD eighth
        for ray in {R * x // 8, max(R * (x + 1) // 8 - 1, 0)}:
            assert all(np.isfinite(a[ray]).all() for a in (*ws, *sps, *eus)), f"ray {ray} (eighth {x}) is stale"
    r = _check_stages(ops, props, o, d, area, nears, fars, counts, pad, ws, sps, eus, f"fused R={R}")
    print(f"fused R={R}: euclid0 {r[0]:.3g}, weights {r[1]:.3g}, DELTA share {r[2]:.3g}, euclid {r[3]:.3g}")


@pytest.mark.parametrize("inline", ["0", "1"])
def test_fused_sampler_with_actors_bins(ops, monkeypatch, switches, inline):
    """nrhip_proposal_sampler_fwd_actors under both NRHIP_SAMPLER_ACTOR_INLINE settings: stages 1 and 3 (the brackets do
    not depend on how the densities were formed; the actor densities themselves are tests/test_gpu_actors.py's)"""
    from neurad_studio_amd.fields.neurad_field import NeuRADProposalField, NeuRADProposalFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    switches.set("NRHIP_SAMPLER_ACTOR_INLINE", inline)
    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    c = NeuRADProposalFieldConfig()
    c.grid.static.log2_hashmap_size, c.grid.actor.log2_hashmap_size = 11, 8
    p = NeuRADProposalField(c, actors=actors, static_scale=100.0).cuda().eval()
    ref = SR.sharp_prop(95)
    with torch.no_grad():
        p.hashgrid.static_grid.hash_table.copy_(cuda(ref.grid.table))
        for i, gr in enumerate(p.hashgrid.actor_grids):
            gr.hash_table.copy_(cuda(synth.hash_table(gr.hash_table.shape[0], 1, seed=500 + i, scale=1.5)))
        p.density_decoder.weight.copy_(cuda(ref.decoder_w))
    assert p.fused_sampler_supported()
    fields = [p, p]  # both rounds evaluate the last proposal field, as the model's eval path does (one actor set)
    rb = actor_rays(101)
    R, counts, pad = 101, (130, 65, 33), 0.0
    o, d, area, times = rb.origins, rb.directions, rb.pixel_area.reshape(-1), rb.times.reshape(-1)
    nears = torch.zeros(R, device="cuda")
    _, cand = fields[0].hashgrid.prepare_actors(o, d, area, torch.stack([nears, nears + 1], -1),
                                                torch.stack([nears + 1, nears + 2], -1), times)
    assert int((cand[0] > 0).sum()) > R // 2  # most rays meet an actor
    fars = np.full(R, 300.0, np.float32)
    ws, sps, eus = _fused(ops, monkeypatch, [f.proposal_spec() for f in fields], False, host(o), host(d), host(area), None,
                          fars, counts, pad, actor_specs=[f.hashgrid.actor_spec() for f in fields], cand=cand)
    r = _check_stages(ops, None, host(o), host(d), host(area), None, fars, counts, pad, ws, sps, eus,
                      f"fused actors inline={inline}", stage2=False)
    print(f"fused actors inline={inline}: euclid0 {r[0]:.3g}, DELTA share {r[2]:.3g}, euclid {r[3]:.3g}")


# ---- D. fused against unfused ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad,factor", [(0.01, SR.SHARP), (0.0, SR.SHARP), (0.01, SR.OPAQUE)],
                         ids=["pad0.01_x12", "pad0.0_x12", "pad0.01_x20"])
def test_fused_and_unfused_chain_agree_on_the_sharp_field(ops, monkeypatch, pad, factor):
    counts = (128, 64, 32)
    props = SR.variant_props((6, 6), False, factor)
    o, d, area, nears, fars = SR.variant_inputs(SR.R, True, None)
    far_used = np.full(SR.R, SKY, np.float32)
    ws, sps, eus = _fused(ops, monkeypatch, props, False, o, d, area, nears, fars, counts, pad)
    r = _check_stages(ops, props, o, d, area, nears, fars, counts, pad, ws, sps, eus, "fused")
    print(f"fused pad={pad} x{factor:g}: euclid0 {r[0]:.3g}, weights {r[1]:.3g}, DELTA share {r[2]:.3g}, euclid {r[3]:.3g}")
    # the operator chain, each kernel held to the same references on its own inputs
    sp, eu = ops.power_sampler(dev(nears), dev(far_used), counts[0])
    cw, csp, ceu = [], [host(sp)], [host(eu)]
    for k, p in enumerate(props):
        dens = ops.proposal_density_fwd(to_pspec(ops, p), dev(o), dev(d), dev(area), eu[:, :-1].contiguous(), eu[:, 1:].contiguous())
        rdens = O.proposal_density(p, o, d, area, ceu[k][:, :-1], ceu[k][:, 1:]).astype(np.float64)
        rel = np.abs(host(dens).astype(np.float64) / rdens - 1)
        print(f"chain pad={pad} x{factor:g} round {k}: density err / rho {float(rel.max() / SR.prop_rho(p)):.3g}")
        assert (rel <= SR.prop_rho(p)).all(), f"density round {k}: relative error {rel.max():.3g} > rho {SR.prop_rho(p):.3g}"
        w = ops.weights_from_density((eu[:, 1:] - eu[:, :-1]).contiguous(), dens)
        sp, eu = ops.pdf_sample(w, sp, dev(nears), dev(far_used), counts[k + 1], histogram_padding=pad)
        cw.append(host(w)), csp.append(host(sp)), ceu.append(host(eu))
    r = _check_stages(ops, props, o, d, area, nears, fars, counts, pad, cw, csp, ceu, "chain")
    print(f"chain pad={pad} x{factor:g}: euclid0 {r[0]:.3g}, weights {r[1]:.3g}, DELTA share {r[2]:.3g}, euclid {r[3]:.3g}")
    # the final euclidean bins of the two paths: within the sum of their two bounds, the spacing bracket of each path's
    # last round carried through the euclidean bound at its ends
    width = 0.0
    for w_, s_, in ((ws, sps), (cw, csp)):
        lo, hi, _ = SR.bracket(w_[-1], s_[-2], counts[-1], pad, None)
        elo, _, _ = SR.euclid_bounds(np.clip(lo, 0.0, 1.0), nears, far_used)
        _, ehi, _ = SR.euclid_bounds(np.clip(hi, 0.0, 1.0), nears, far_used)
        width = width + (ehi - elo)
    diff = np.abs(eus[-1].astype(np.float64) - ceu[-1].astype(np.float64))
    print(f"fused vs chain pad={pad}: max |difference| / (sum of the two bounds) = {float((diff / width).max()):.3g}")
    over = diff > width
    assert not over.any(), f"{int(over.sum())} final edges differ by more than both bounds, first {tuple(np.argwhere(over)[0])}"
