"""The bracket reference of tests/sampler_refs.py is right and sharp, shown on the CPU with plain numpy: three correct
evaluations of the resampler (the oracle's, a sequential and a pairwise fp32 running sum) lie inside every bracket, and
every one-defect variant is flagged on the input family that reaches the defect."""
import numpy as np
import pytest

import neurad_oracle as O
import sampler_refs as SR

f32 = np.float32


def _cumsum32(pdf, how):
    if how == "oracle":  # float64 accumulation, each output rounded (torch.cumsum on the CPU)
        return np.cumsum(pdf.astype(np.float64), -1).astype(f32)
    if how == "seq":
        return np.cumsum(pdf.astype(f32), -1, dtype=f32)
    if how == "chunks":  # DEFECT: the running sum restarted at every 64th weight
        out = np.empty_like(pdf)
        for k0 in range(0, pdf.shape[-1], 64):
            out[..., k0:k0 + 64] = np.cumsum(pdf[..., k0:k0 + 64], -1, dtype=f32)
        return out
    n = pdf.shape[-1]  # pairwise: the halves' running sums, the right one shifted by the left one's total
    if n <= 1:
        return pdf.astype(f32)
    left, right = _cumsum32(pdf[..., : n // 2], how), _cumsum32(pdf[..., n // 2:], how)
    return np.concatenate([left, (right + left[..., -1:]).astype(f32)], -1)


def pdf_sample_variant(case, cumsum="oracle", defect=None):
    """oracle/neurad_oracle.py::pdf_sample's arithmetic (fp32) with the running sum's order as a parameter and, optionally,
    exactly one defect -> new spacing bins"""
    w, bins, Sn, pad, rand = case["w"], case["bins"], case["Sn"], case["pad"], case["rand"]
    R, Sp = w.shape
    w = w + f32(0.0 if defect == "no_pad" else pad)
    wsum = w.sum(-1, keepdims=True, dtype=f32)
    padding = np.zeros_like(wsum) if defect == "no_eps" else np.maximum(f32(1e-5) - wsum, f32(0))
    w = w + padding / f32(Sp)
    wsum = wsum + padding
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = (w / wsum).astype(f32)
    cdf = np.minimum(f32(1), _cumsum32(pdf, "chunks" if defect == "lost_carry" else cumsum))
    cdf = np.concatenate([np.zeros_like(cdf[..., :1]), cdf], -1)
    nb = Sn + 1
    u = O.linspace(0.0, 1.0 - (1.0 / nb), nb)
    if rand is not None:
        rr = np.asarray(rand, f32).reshape(R, -1)
        if defect == "jitter_stride" and rr.shape[1] > 1:  # per-bin jitter read with the single-jitter stride
            rr = rr.reshape(-1)[:R, None]
        if defect == "jitter_prev_ray":
            rr = np.roll(rr, 1, 0)
        u = u[None, :] + rr / f32(nb)
    elif defect != "no_offset":
        u = u + f32(1.0 / (2 * nb))
    u = np.broadcast_to(u, (R, nb)).astype(f32)
    side = "left" if defect == "left" else "right"
    inds = np.stack([np.searchsorted(cdf[r], u[r], side=side) for r in range(R)]) + (1 if defect == "shift" else 0)
    below, above = np.clip(inds - 1, 0, Sp), np.clip(inds, 0, Sp)
    c0, c1 = np.take_along_axis(cdf, below, -1), np.take_along_axis(cdf, above, -1)
    b0, b1 = np.take_along_axis(bins, below, -1), np.take_along_axis(bins, above, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (u - c0) / (c1 - c0)
        if defect != "nan_kept":
            t = np.nan_to_num(t, nan=0.0, posinf=np.inf, neginf=-np.inf)
        if defect != "no_clip":
            t = np.clip(t, 0, 1)
        return (b0 + t.astype(f32) * (b1 - b0)).astype(f32)


@pytest.fixture(scope="module")
def all_cases():
    out = []
    for c in SR.cases():
        lo, hi, mid = SR.bracket(c["w"], c["bins"], c["Sn"], c["pad"], c["rand"])
        out.append((c, lo, hi, mid))
    return out


def test_every_bracket_is_sharp(all_cases):
    assert len(all_cases) == len(SR.COUNTS) * 2 * 3 * 2 * 2 + 2
    for c, lo, hi, _ in all_cases:
        assert (lo <= hi).all()
        SR.assert_sharp(lo, hi, c["Sn"], c["name"])


@pytest.mark.parametrize("cumsum", ["oracle", "seq", "pairwise"])
def test_correct_evaluations_lie_inside(all_cases, cumsum):
    worst = 0.0
    for c, lo, hi, mid in all_cases:
        got = pdf_sample_variant(c, cumsum)
        if cumsum == "oracle":  # the restatement above IS the oracle's arithmetic
            sp = O.Spacing(f32(0), f32(1), -1.0, 0.1)
            want, _ = O.pdf_sample(c["w"], c["bins"], c["Sn"], sp, c["pad"],
                                   rand=None if c["rand"] is None else c["rand"].reshape(SR.R, -1))
            assert np.array_equal(got, want), c["name"]
        SR.check_bracket(got, lo, hi, f"{cumsum}: {c['name']}")
        SR.check_monotone(got, f"{cumsum}: {c['name']}")
        worst = max(worst, SR.delta_used(got, c["w"], c["bins"], c["Sn"], c["pad"], c["rand"]))
    print(f"pdf_sample[{cumsum}]: max share of DELTA used = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("lam", [-1.0, 0.0, 1.0, -2.0, 0.5])
def test_oracle_spacing_lies_inside_the_euclidean_bound(lam):
    worst = 0.0
    for S, far, seed in ((1, 200.0, 1), (37, 20000.0, 2), (128, 20000.0, 3), (64, 3.5, 4)):
        nears = SR.synth.uniform((SR.R,), 0.5, 3.0, seed)
        fars = np.full((SR.R,), far, f32)
        for n in (None, nears):
            t_rand = SR.synth.uniform((SR.R, S + 1), 0.0, 1.0, seed + 9)
            for tr in (None, t_rand):
                sp, eu, _ = O.power_sampler(np.zeros(SR.R) if n is None else n, fars, S, lam, 0.1, tr)
                assert np.isfinite(eu).all()
                worst = max(worst, SR.check_euclid(eu, sp, n, fars, f"lam={lam} S={S} far={far}", lam, 0.1))
    print(f"Spacing[lam={lam}]: max |got - centre| / bound width = {worst:.3g}")


def test_euclidean_bound_is_per_element_not_uniform():
    """lam = -1, far = 20000: the map turns one ulp of its argument into ~1e-4 relative at the far end and into ~1e-7
    near the origin, and the bound says so"""
    fars = np.full((SR.R,), 20000.0, f32)
    sp, eu, _ = O.power_sampler(np.zeros(SR.R), fars, 128)
    lo, hi, mid = SR.euclid_bounds(sp, None, fars)
    rel = (hi - lo)[:, 1:] / mid[:, 1:]
    assert rel[:, 0].max() < 1e-4 and 1e-4 < rel[:, -1].max() < 1e-2, (rel[:, 0].max(), rel[:, -1].max())
    assert (hi - lo)[:, 0].max() < 1e-4  # metres at the origin: the cancelling `- 1`


def _flagged(all_cases, defect, cumsum="oracle", only=lambda c: True):
    """-> [(case name, rays flagged)] of a one-defect variant"""
    out = []
    for c, lo, hi, _ in all_cases:
        if not only(c):
            continue
        got = pdf_sample_variant(c, cumsum, defect).astype(np.float64)
        bad = ~np.isfinite(got) | (got < lo) | (got > hi)
        if bad.any():
            out.append((c["name"], sorted(set(np.argwhere(bad)[:, 0].tolist()))))
    return out


def _counts(c):
    return c["w"].shape[1], c["Sn"]


def test_defects_are_flagged(all_cases):
    """each variant carries ONE defect; the bracket flags it on the family named here"""
    n_rand = lambda k: lambda c: (c["rand"] is None) if k == "none" else (c["rand"] is not None and c["rand"].ndim == k)
    # (a) the eval-mode offset 1 / (2 nb) left out: every eval-mode case, on the smooth rays too
    hit = _flagged(all_cases, "no_offset", only=n_rand("none"))
    assert len(hit) == sum(c["rand"] is None for c, *_ in all_cases) and all(6 in rays for _, rays in hit), hit[:3]
    # (b) the chunk carry lost: exactly the cases with more than 64 weights, on the ray of ties (7) and on the one-hot and
    #     two-bin rays at the chunk boundary (11, 12) every time
    hit = _flagged(all_cases, "lost_carry")
    big = [c["name"] for c, *_ in all_cases if _counts(c)[0] > 64]
    assert [n for n, _ in hit] == big and all({7, 11, 12} <= set(rays) for _, rays in hit)
    # (c) histogram_padding dropped: the cases with padding, on the one-hot rays (their flat stretches come back);
    #     the eps padding dropped: the empty ray (4) at pad = 0, and nowhere else
    hit = _flagged(all_cases, "no_pad", only=lambda c: c["pad"] > 0 and _counts(c)[0] > 1)
    assert len(hit) == sum(c["pad"] > 0 and _counts(c)[0] > 1 for c, *_ in all_cases) and all(2 in rays for _, rays in hit)
    hit = _flagged(all_cases, "no_eps")
    assert [n for n, _ in hit] == [c["name"] for c, *_ in all_cases if c["pad"] == 0.0] and all(r == [4] for _, r in hit)
    # (d) below / above shifted by one: every case with more than one existing bin
    hit = _flagged(all_cases, "shift", only=lambda c: _counts(c)[0] > 1)
    assert len(hit) == sum(_counts(c)[0] > 1 for c, *_ in all_cases)
    # (e) per-bin jitter read with the single-jitter stride; ray r reading ray r - 1's jitter
    hit = _flagged(all_cases, "jitter_stride", only=n_rand(2))
    assert len(hit) == sum(n_rand(2)(c) for c, *_ in all_cases)
    hit = _flagged(all_cases, "jitter_prev_ray", only=lambda c: c["rand"] is not None)
    assert len(hit) == sum(c["rand"] is not None for c, *_ in all_cases)
    # (f) nan not zeroed: the query that reaches u = 1.0 under a jitter of 1 - 2^-24 (below = above = Sp, 0 / 0), ray 1
    hit = _flagged(all_cases, "nan_kept", only=lambda c: c["rand"] is not None)
    assert len(hit) == sum(c["rand"] is not None for c, *_ in all_cases) and all(1 in rays for _, rays in hit)
    #     t not clipped: a sequential fp32 running sum that ends below 1 under such a query, (u - c) / 0 = inf
    hit = _flagged(all_cases, "no_clip", cumsum="seq", only=lambda c: c["rand"] is not None)
    assert hit and all(set(rays) <= {1, 3} for _, rays in hit), hit[:3]
    # (g) side="left": u = 0 exactly (jitter 0.0) on the one-hot ray whose CDF starts with a flat stretch (ray 2), pad = 0
    hit = _flagged(all_cases, "left", only=lambda c: c["rand"] is not None and c["pad"] == 0.0 and _counts(c)[0] > 2)
    assert len(hit) == sum(c["rand"] is not None and c["pad"] == 0.0 and _counts(c)[0] > 2 for c, *_ in all_cases)
    assert all(2 in rays for _, rays in hit)


# ---- the fused sampler's sharp proposal fields ---------------------------------------------------------------------------
def _oracle_chain(props, R, counts, pad, nears=None, fars=None):
    o, d, area = SR.sharp_rays(R)
    nears = np.zeros(R, f32) if nears is None else nears
    fars = np.minimum(np.full(R, 20000.0, f32) if fars is None else fars, f32(20000.0))
    bins, eu, sp = O.power_sampler(nears, fars, counts[0])
    rounds = []
    for k, p in enumerate(props):
        dens = O.proposal_density(p, o, d, area, eu[:, :-1], eu[:, 1:])
        w = O.weights_from_density(eu[:, 1:] - eu[:, :-1], dens)
        nbins, neu = O.pdf_sample(w, bins, counts[k + 1], sp, pad)
        rounds.append(dict(eu=eu, bins=bins, dens=dens, w=w, new_bins=nbins, new_eu=neu))
        bins, eu = nbins, neu
    return rounds


def test_sharp_fields_are_sharp_and_their_brackets_too():
    """SR.SHARP is the smallest of the factors tried at which the log-densities pass +-15 and more than a third of the
    rays have one bin with w > 0.9; the oracle's own chain lies inside the brackets taken from its own weights, which
    meet the 99 % condition at both paddings"""
    props = lambda f: [SR.sharp_prop(91, factor=f), SR.sharp_prop(95, factor=f)]
    o, d, area = SR.sharp_rays(SR.R)

    def sharp_enough(f):
        rounds = _oracle_chain(props(f), SR.R, (128, 64, 32), 0.01)
        acc = np.log(np.concatenate([r["dens"].ravel() for r in rounds]).astype(np.float64))
        return all(3 * (r["w"].max(-1) > 0.9).sum() >= SR.R for r in rounds) and acc.min() < -15 and acc.max() > 15

    assert [f for f in (4.0, 8.0, 12.0, 16.0) if sharp_enough(f)][0] == SR.SHARP
    runs = [(SR.R, v, i) for v, i in zip(SR.VARIANTS, SR.VARIANT_IDS)]
    runs += [(R, ((16, 8, 4), (6, 6), False, True, None, 0.01, SR.SHARP), f"R={R}") for R in (1, 5, 33, 300)]
    for R, (counts, levels, half, with_nears, fars_kind, pad, factor), vid in runs:
        ps = SR.variant_props(levels, half, factor)
        _, _, _, nears, fars = SR.variant_inputs(R, with_nears, fars_kind)
        far_used = np.minimum(np.full(R, 20000.0, f32) if fars is None else fars, f32(20000.0))
        for k, r in enumerate(_oracle_chain(ps, R, counts, pad, nears, fars)):
            what = f"oracle chain {vid} round {k}"
            lo, hi, _ = SR.bracket(r["w"], r["bins"], counts[k + 1], pad, None)
            SR.assert_sharp(lo, hi, counts[k + 1], what)
            SR.check_bracket(r["new_bins"], lo, hi, what)
            SR.check_euclid(r["new_eu"], r["new_bins"], nears, far_used, what)
            SR.check_weights(r["w"], r["eu"], r["dens"], SR.prop_rho(ps[k]), what)


def test_c_oracle_weights_lie_inside_the_stage2_bound_built_on_rho():
    """oracle/neurad_oracle_c.c evaluates the proposal density on its own (its own cube roots, summation order and expf) but
    hands out only the sampler chain's weights, not the densities: so rho is confirmed through them -- its first-round
    weights, on the same bit-identical power bins, lie within the stage-2 bound built on the numpy oracle's densities, at
    the sharp field and at the unscaled one.  This is weaker than a density comparison (on the sharp field the weights use
    0.002 of the bound: most of it is the transmittance term); the direct |density / oracle - 1| <= rho assertion is made
    where a second density evaluation exists, on ops.proposal_density_fwd (tests/test_gpu_sampler_sharp.py, section D)."""
    import oracle_c

    o, d, area = SR.sharp_rays(SR.R)
    for factor in (SR.SHARP, 1.0):
        props = [SR.sharp_prop(91, factor=factor), SR.sharp_prop(95, factor=factor)]
        r0 = _oracle_chain(props, SR.R, (128, 64, 32), 0.01)[0]
        c = oracle_c.proposal_sampler(props, o, d, area, np.zeros(SR.R, f32), np.full(SR.R, 20000.0, f32),
                                      late_binding_quirk=False)
        assert np.array_equal(np.concatenate([c["prop_starts"][0], c["prop_ends"][0][:, -1:]], -1), r0["eu"])
        ratio = SR.check_weights(c["prop_weights"][0], r0["eu"], r0["dens"], SR.prop_rho(props[0]), f"C oracle x{factor}")
        print(f"C oracle vs numpy oracle, decoder x{factor}: max err / bound = {ratio:.3g}")
