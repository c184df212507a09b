"""tests/loss_refs.py on the CPU: the restated radix select against torch.quantile bit for bit, the fp64 lidar reference
against the package's torch formulation with autograd, and the proof that the case lists of
tests/test_gpu_loss_kernels.py tell a correct kernel from the plausible wrong ones."""
import numpy as np
import pytest
import torch

import loss_refs as LR
import neurad_oracle as O
from conftest import rel_l2

CASES = LR.lidar_cases()


def _quantile_inputs():
    """(name, err, q): the error vector of every lidar case, and the issue's grid on synthetic inputs"""
    out = [(name, LR.lidar_ref(c)["err"].numpy(), c["q"]) for name, c in CASES.items()]
    rs = np.random.RandomState(0)
    for n in (1, 2, 3, 21, 300, 4097, 40000):
        kinds = {"random": rs.uniform(0, 100, n).astype(np.float32),
                 "three_valued": rs.choice(np.array([1.5, 2.5, 40.0], np.float32), n),
                 "low_byte": LR.byte_errors(0, n, seed=n), "top_nibble": LR.byte_errors(3, n, seed=n)}
        for kind, e in kinds.items():
            out += [(f"{kind}_{n}_q{q}", e, q) for q in (0.0, 0.05, 0.5, 0.95, 0.999, 1.0)]
    return out


def test_radix_threshold_is_torch_quantile_bit_for_bit():
    inputs = _quantile_inputs()
    assert len(inputs) > 180
    for name, e, q in inputs:
        want = torch.quantile(torch.from_numpy(e), q).numpy()
        got = LR.radix_threshold(e, q)
        assert LR.bits(got) == LR.bits(want), (name, float(got), float(want))


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c["n"] <= 300])
def test_lidar_ref_agrees_with_the_torch_formulation(name):
    """lidar_metrics(fused=False) in fp32 with autograd; where the kept set or the returned kept set is empty the metric is
    0 / 0 on both sides and autograd's 0 * inf gradient is not compared (loss_refs defines it as zero).  An infinite error
    outside the kept set leaves the mean of the kept errors finite (models/neurad.py:499 indexes, and so do the kernel and
    loss_refs); the masked product of the torch formulation makes it inf * 0, so that term is not compared there."""
    c = CASES[name]
    ref = LR.lidar_ref(c)
    vals, gd, gi, gl = LR.lidar_metrics_cpu(c)
    finite = bool(torch.isfinite(ref["err"]).all())
    assert finite or name.startswith("mixed_inf")
    for k in range(2 + c["levels"]):
        if k == 0 and not finite:
            assert np.isfinite(float(ref["metrics"][0]))
            continue
        a, b = float(vals[k]), float(ref["metrics"][k])
        assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 2e-5 * abs(b), (k, a, b)
    if ref["n_keep"] and finite:
        assert rel_l2(gd[0].numpy(), ref["gdepth"][0].numpy()) < 2e-5
    if ref["n_sel"]:
        assert rel_l2(gi.numpy(), ref["gint"].numpy()) < 2e-5
    assert rel_l2(gl.numpy(), ref["glogit"].numpy()) < 2e-5
    for l in range(1, c["levels"]):
        assert rel_l2(gd[l].numpy(), ref["gdepth"][l].numpy()) < 2e-5
    # exact zeros: camera rows, rays outside the kept set, beams without a return in the intensity gradient
    for g in ref["gdepth"]:
        assert float(g[~c["is_lidar"]].abs().max()) == 0.0
    assert float(ref["gdepth"][0][c["rows"]][~ref["keep"]].abs().sum()) == 0.0
    assert float(ref["gint"][~(ref["keep"] & c["did_return"])].abs().sum()) == 0.0


def test_large_lidar_cases_agree_with_the_torch_formulation():
    """the size branches above 300 rays: the values only (their gradients follow the same code as the small cases)"""
    for name, c in CASES.items():
        if c["n"] > 300:
            ref = LR.lidar_ref(c)
            vals = LR.lidar_metrics_cpu(c)[0]
            assert rel_l2(vals.numpy(), ref["metrics"].numpy()) < 2e-5, name


def test_degenerate_sampler_case_is_nan_in_the_reference_on_ray_0_only():
    c, w, cp, wp = LR.degenerate_sampler_case()
    with np.errstate(all="ignore"):
        loss, _, grad = O.interlevel_loss_level(c, w, cp, wp, LR.PULSE)
    assert np.isnan(loss[0]) and np.isfinite(loss[1:]).all() and np.isfinite(grad[1:]).all()


def _lidar_signature(c, variant):
    r = LR.lidar_ref(c, variant)
    return LR.bits(r["err"]).tobytes(), LR.bits(r["thr"]).tobytes(), r["keep"].numpy().tobytes()


@pytest.mark.parametrize("variant", LR.LIDAR_VARIANTS)
def test_lidar_cases_tell_the_wrong_variant(variant):
    hit = [n for n, c in CASES.items() if _lidar_signature(c, variant) != _lidar_signature(c, None)]
    assert hit, variant
    # with no variant the restated select IS the reference's threshold, so the comparison above is like for like
    for n in hit[:3]:
        r = LR.lidar_ref(CASES[n])
        assert LR.bits(LR.radix_threshold(r["err"].numpy(), CASES[n]["q"])) == LR.bits(r["thr"])


def _carving_inputs(c, did_return=True):
    S = c["S"]
    return (c["edges"][:, :S], c["edges"][:, 1:S + 1], c["is_lidar"], c["did_return"] if did_return else None,
            c["distance"], LR.EPS, LR.NON_RETURN)


@pytest.mark.parametrize("variant", LR.CARVING_VARIANTS)
def test_carving_cases_tell_the_wrong_variant(variant):
    hit = 0
    for R, S in LR.CARVING_SHAPES:
        c = LR.carving_case(R, S)
        hit += not torch.equal(LR.carving_ref(*_carving_inputs(c), variant=variant)[0], LR.carving_ref(*_carving_inputs(c))[0])
    assert hit, variant


def test_carving_cases_sit_on_the_band_edges_and_are_exact():
    Rs, Ss = {s[0] for s in LR.CARVING_SHAPES}, {s[1] for s in LR.CARVING_SHAPES}
    assert Rs == {1, 3, 4, 5, 1027} and Ss == {1, 63, 64, 65, 129}
    assert any(R % 4 and S > 64 for R, S in LR.CARVING_SHAPES)
    for R, S in LR.CARVING_SHAPES:
        c = LR.carving_case(R, S)
        on_eps, on_nr = c["share"]
        assert on_eps > 0 and (R == 1 or on_nr > 0), (R, S, c["share"])
        # with did_return absent every lidar ray counts as returned
        assert LR.carving_share(c, c["is_lidar"], torch.ones(R, dtype=torch.bool))[0] > 0
        # exact: the fp64 evaluation of the mask gives the same booleans
        s, e, lid, ret, d, eps, nr = _carving_inputs(c)
        close, loss, grad = LR.carving_ref(s, e, lid, ret, d, eps, nr, c["weights"])
        close64 = LR.carving_ref(s.double(), e.double(), lid, ret, d.double(), eps, nr)[0]
        assert torch.equal(close, close64)
        far = lid[:, None] & ~close
        assert torch.equal(grad, 2 * c["weights"].double() * far) and loss.shape == (R,)
        assert not close[~lid].any()


def test_mask_cases():
    for R in LR.MASK_RS:
        for name, m in LR.mask_cases(R).items():
            rows, inv = LR.compact_ref(m)
            assert m.shape == (R,) and rows.numel() == int(m.sum()), (R, name)
            assert torch.equal(inv >= 0, m) and torch.equal(rows[inv[m].long()], rows)
    assert int(LR.mask_cases(16389)["pass_edges"].sum()) == 4 and int(LR.mask_cases(8192)["pass_edges"].sum()) == 1


def test_sampler_cases_cover_the_chunk_boundaries_and_the_fp64_restatement_is_the_oracle_formula():
    shapes = LR.SAMPLER_SHAPES
    assert {s[0] for s in shapes} == {1, 4, 5, 9} and {s[1] for s in shapes} == {1, 31, 32, 33, 64, 128}
    assert {s[2] for s in shapes} == {1, 63, 64, 65, 128, 512} and (9, 128, 512) in shapes
    assert {(2 * s[1] + 1) % 64 for s in shapes} >= {63, 1} and {(s[2] + 1) % 64 for s in shapes} >= {0, 1, 2}
    for R, sf, sp in shapes:
        c, w, cp, wp = LR.sampler_case(R, sf, sp)
        assert (np.diff(c, axis=-1) >= 0).all() and (np.diff(cp, axis=-1) >= 0).all()
        assert c.min() == 0 and c.max() == 1 and cp.min() == 0 and cp.max() == 1
        loss, _, grad = O.interlevel_loss_level(c, w, cp, wp, LR.PULSE)
        l64, g64 = LR.interlevel_ref64(c, w, cp, wp, LR.PULSE)
        assert np.isfinite(loss).all() and np.isfinite(l64).all()
        # the same formula: most rays agree to fp32 rounding; a ray with a chance narrow fine bin (w / width in the
        # thousands, cancelled again by the cumulative sums) is where the fp32 oracle itself is 1e-4 .. 1e-3 from fp64
        rel = np.abs(loss - l64) / np.abs(l64)
        assert (l64 > 0).all()
        assert np.median(rel) < 2e-5 and rel.max() < 5e-3 and rel_l2(grad, g64) < 5e-3, (R, sf, sp, rel)
        if sp >= 8:
            knots = np.concatenate([c - np.float32(LR.PULSE), c + np.float32(LR.PULSE)], -1)
            on_knot = [(np.isin(cp[i, 1:-1], knots[i])).sum() for i in range(R)]
            assert min(on_knot) >= 1, (R, sf, sp, on_knot)
            assert ((np.diff(cp, axis=-1) == 0).sum(-1) >= 1).all()
