"""The proposal-kernel cases (tests/proposal_refs.py) are what they claim to be, their tolerance helpers hold for an fp32
evaluation with one-ulp transcendentals, and their expected outputs tell the wrong variants of the kernels apart.  No GPU."""
import numpy as np
import pytest

import neurad_oracle as O
import proposal_refs as P
from table_grad_refs import U, bound_for

f32 = np.float32
LEVELS = sorted(P.GRIDS)


@pytest.fixture(scope="module")
def big():
    """one exact case per level count, 683 x 3 samples, with its reference"""
    out = {}
    for L in LEVELS:
        c = P.exact_case(2049, L, seed=1)
        out[L] = (c, P.forward_ref(c))
    return out


@pytest.mark.parametrize("L", LEVELS)
def test_scalings_are_powers_of_two_and_ops_agrees(L):
    from neurad_studio_amd import ops

    mn, mx = P.GRIDS[L]
    s = O.hash_scalings(L, mn, mx)
    assert (np.frexp(s)[0] == 0.5).all() and s[0] == 16 and s[-1] == mx
    assert np.array_equal(ops.GridSpec(L, 1, P.LOG2_T, mn, mx).scalings.numpy(), s)


@pytest.mark.parametrize("L", LEVELS)
def test_exact_family_is_exact(big, L):
    """the oracle's fp32 op-for-op encode_static equals the float64 evaluation bit for bit; positions, offsets and table
    values are fp32 (and fp16) numbers; the rescale weight is 1"""
    c, fwd = big[L]
    enc32 = O.encode_static(c.params().grid, P.STATIC_SCALE, c.o, c.d, c.area, c.edges[:, :-1], c.edges[:, 1:])
    assert enc32.dtype == f32 and np.array_equal(enc32.astype(np.float64), fwd.lf)
    assert np.array_equal(fwd.pos.astype(f32).astype(np.float64), fwd.pos)
    assert np.array_equal(fwd.lf.astype(f32).astype(np.float64), fwd.lf)
    assert np.array_equal(c.table.astype(np.float16).astype(f32), c.table) and np.abs(c.table).max() == 3
    assert (fwd.rw == 1).all() and (fwd.std == 0).all()
    assert (c.dec != 0).all() and len(np.unique(c.dec)) == L and np.array_equal(np.round(c.dec * 8), c.dec * 8)
    t = (c.edges[:, :-1] + c.edges[:, 1:]) / 2
    assert t.max() <= 10 and np.array_equal(np.round(t * 16), t * 16)
    # fp32 lerp tree as the kernels run it (fmaf = one rounding of the exact a * b + c, emulated in float64): also exact
    ox = (fwd.pos[:, None, :] * c.scalings[None, :, None].astype(np.float64)) % 1.0
    assert np.abs(ox * 2 ** 21 - np.round(ox * 2 ** 21)).max() == 0  # 7 bits per axis at scaling 16: the products fit


def test_regime_shares_and_zero_offsets(big):
    for L in LEVELS:
        c, fwd = big[L]
        inside, face2, face1 = fwd.mag < 1, fwd.mag == 2, fwd.mag == 1
        assert (inside | face2 | face1).all()
        assert inside.mean() >= 0.7 and face2.mean() >= 0.1 and face1.mean() >= 0.1
        assert np.array_equal(np.repeat(c.regime, c.S), np.where(inside, P.INSIDE, np.where(face2, P.FACE2, P.FACE1)))
        # contraction: on the 2 * scale face the face coordinate lands on 1/8 or 7/8, on the scale face on 1/4 or 3/4
        assert np.isin(fwd.pos[face2], [0.125, 0.875]).any(-1).all() and np.isin(fwd.pos[face1], [0.25, 0.75]).any(-1).all()
        _, off = O.hashgrid_corner_indices(fwd.pos.astype(f32), c.scalings, 1 << P.LOG2_T)
        zero = (off == 0).mean((0, 2))  # per level
        assert (zero >= 1 / 16).all(), zero  # offsets of 0 (floor == ceil) at every level, the coarsest included
        assert ((off == 0).all(-1).sum(0) > 0).all()  # and samples with all three at once


def test_rescaled_family_crosses_one_in_both_zones():
    c = P.rescaled_case(2049, 6, seed=1)
    fwd = P.forward_ref(c)
    exact = P.forward_ref(P.exact_case(2049, 6, seed=1))
    assert np.array_equal(fwd.pos, exact.pos) and np.array_equal(fwd.interp, exact.interp)
    arg = 2 * c.scalings[None, :].astype(np.float64) * fwd.std[:, None]
    for zone in (fwd.mag < 1, fwd.mag == 1, fwd.mag == 2):
        assert (arg[zone, 0] < 1).mean() > 0.8 and (arg[zone, -1] > 1).mean() > 0.8
        assert ((fwd.rw[zone] < 1).any(1) & (fwd.rw[zone] == 1).any(1)).mean() > 0.8


def test_rtol_rw_holds_for_one_ulp_transcendentals():
    """the kernels' std and rescale weight, op for op in fp32 with numpy's log2 / exp2 (within one ulp): inside the bound;
    and the bound is what common.h calls '~1e-6', not a loose one"""
    c = P.rescaled_case(2049, 6, seed=1)
    fwd = P.forward_ref(c)
    t0, t1 = c.edges[:, :-1], c.edges[:, 1:]
    dist = (t1 - t0) / f32(2)
    t = t0 + dist

    def cbrt32(x):
        return np.exp2(np.log2(x.astype(f32)) * f32(1.0 / 3.0)).astype(f32)

    std = (cbrt32((c.area[:, None] * (t * t)) * dist) / f32(P.STATIC_SCALE)).reshape(-1)
    cm = np.maximum(fwd.mag, 1).astype(f32)
    sc = cbrt32(f32(2) * cm - f32(1)) / cm
    std = np.where(fwd.mag < 1, std, std * (sc * sc)) / f32(4)
    assert std.dtype == f32
    rw = f32(1) / np.maximum(c.scalings[None, :] * f32(2) * std[:, None], f32(1))
    lf = fwd.interp.astype(f32) * rw
    bound = P.rtol_rw(c, fwd)
    err = np.abs(lf.astype(np.float64) - fwd.lf)
    assert (err <= bound * np.abs(fwd.lf)).all()
    assert bound.min() > 2 * P.E and bound.max() < 2e-6
    wrong = fwd.interp / np.maximum(2.0 * c.scalings[None, :] * fwd.std[:, None] * (1 + 1e-5), 1.0)  # a std off by 1e-5
    assert (np.abs(wrong - fwd.lf) > bound * np.abs(fwd.lf)).any()


def test_density_and_gx_bounds_hold_in_fp32():
    c = P.saturation_case(2049, 6, seed=2)
    fwd = P.forward_ref(c)
    acc = np.zeros(c.n, f32)
    for l in range(c.L):
        acc = acc + fwd.lf[:, l].astype(f32) * c.dec[0, l]
    with np.errstate(over="ignore", divide="ignore"):
        dens = np.exp(acc)
        ok = np.isfinite(dens) & (dens >= np.finfo(f32).tiny)  # (a subnormal density has fewer bits)
        assert (np.abs(dens.astype(np.float64) - np.exp(fwd.x))[ok] <= P.density_bound(c, fwd)[ok]).all()
        g = P.saturation_grad(fwd, seed=2)
        gx = g * np.exp(np.clip(np.log(dens), f32(-15), f32(15)))
    ref = P.backward_ref(c, fwd, g)
    assert gx.dtype == f32 and np.isfinite(gx).all()
    assert (np.abs(gx.astype(np.float64) - ref.gx) <= P.gx_rtol(c, fwd) * np.abs(ref.gx)).all()
    assert P.gx_rtol(c, fwd)[np.abs(fwd.x) > 16].max() <= 18 * 2 * P.E  # beyond the clamp: no logit term


def test_saturation_case_covers_the_clamp():
    c = P.saturation_case(2049, 6, seed=2)
    fwd = P.forward_ref(c)
    x = fwd.x
    with np.errstate(over="ignore"):
        d32 = np.exp(x).astype(f32)
    tiny = np.finfo(f32).tiny
    for lo, hi in ((0, 14), (14, 15), (15, 16.5), (16.5, 88)):
        assert ((x > lo) & (x < hi)).sum() >= 3 and ((x < -lo) & (x > -hi)).sum() >= 3, (lo, hi)
    assert (x == 0).sum() >= 1 and (np.abs(x) == 16).sum() >= 1
    assert np.isinf(d32).sum() >= 4 and (d32 == 0).sum() >= 1 and ((d32 > 0) & (d32 < tiny)).sum() >= 1
    g = P.saturation_grad(fwd, seed=2)
    assert ((g == 0) & np.isinf(d32)).sum() >= 2 and ((g != 0) & np.isinf(d32)).sum() >= 2
    ref = P.backward_ref(c, fwd, g)
    assert np.isfinite(ref.ddec).all() and np.isfinite(ref.table).all()


def test_nan_case_poisons_a_known_set():
    c, bad = P.nan_case(1025, 6, seed=3)
    fwd = P.forward_ref(c)
    assert 2 <= len(bad) < c.n // 4 and np.isnan(c.table).sum() == 1
    assert np.array_equal(np.flatnonzero(np.isnan(fwd.x)), bad)
    assert np.isnan(fwd.lf[bad, 0]).all() and np.isfinite(fwd.lf[:, 1:]).all()
    g = P.grad_with_silent_windows(c.n, seed=3)
    g[bad] = 0.5
    ref = P.backward_ref(c, fwd, g)
    assert np.isnan(ref.ddec).all()
    want = np.zeros(ref.table.shape, bool)
    want[fwd.idx[bad].reshape(-1)] = True
    assert np.array_equal(np.isnan(ref.table), want) and want.sum() >= 8 * c.L
    assert np.isfinite(ref.atomic_bound()[~want]).all()


# ---- the launch arithmetic ----------------------------------------------------------------------------------------------------
LP_SIZES = (1, 3, 1023, 1024, 1025, 2049)


def test_lp_plan_of_the_forward_sizes():
    assert [P.lp_plan(n, 6)[0] for n in LP_SIZES] == [256, 256, 256, 256, 512, 768]
    assert [P.lp_plan(1025, L)[2] for L in (1, 2, 3, 6)] == [4, 8, 12, 24]  # units over 8 slots: half, one, 1.5, 3 rounds
    assert P.lp_plan(2049, 6)[1] == 3  # three blocks per unit
    for n in LP_SIZES:
        for L in (1, 2, 3, 6):
            assert (P.lp_writes(n, L) == 1).all(), (n, L)


@pytest.mark.parametrize("variant", ["hi-1", "drop-first", "unit-round"])
def test_lp_sizes_tell_the_wrong_partition(variant):
    """a quarter's `hi` off by one, a sample dropped at a quarter boundary, an incomplete round of units dropped: each leaves
    an element of the NaN-prefilled level features unwritten at one of the tested sizes (and which ones is stated)"""
    missed = {(n, L) for n in LP_SIZES for L in (1, 2, 3, 6) if (P.lp_writes(n, L, variant) != 1).any()}
    if variant == "hi-1":
        assert {(1024, 1), (1025, 6), (1, 1)} <= missed
        assert (P.lp_writes(1024, 1, variant) == 0).sum() == 4  # four exactly full quarters, each one short
    elif variant == "drop-first":
        assert {(1024, 6), (2049, 6)} <= missed and (1, 6) not in missed and (3, 6) not in missed
        assert np.flatnonzero(P.lp_writes(1025, 1, variant)[0] == 0).tolist() == [512, 1024]  # 1024: a quarter of one sample
    else:
        assert missed == {(n, L) for n in LP_SIZES for L in (1, 3)}  # 4 and 12 units: a partial round


def test_stride_case_reaches_the_second_pass():
    for n, L, vec in ((2049 * 129, 6, 1), (4105 * 256, 2, 4)):
        lf, g, chosen, ddec = P.stride_case(n, L, vec)
        per_pass = 1024 * 256 * vec
        assert n % 4 == (0 if vec == 4 else 1) and per_pass < n < per_pass + per_pass // 64
        assert {0, per_pass - 1, per_pass, n - 1, 256 * vec - 1, 256 * vec} <= set(chosen.tolist())
        assert (g[chosen] != 0).all() and np.count_nonzero(g) == len(chosen) <= 64
        # a kernel that stops after its first pass, or runs the second pass's first thread twice, gives another sum
        first = (lf[:, chosen[chosen < per_pass]].astype(np.float64) * g[chosen[chosen < per_pass]]).sum(1)
        assert (first != ddec).any()
        assert ((ddec + lf[:, per_pass].astype(np.float64) * g[per_pass]) != ddec).any()
        assert np.array_equal(ddec.astype(f32).astype(np.float64), ddec)


# ---- wrong variants of the references -------------------------------------------------------------------------------------------
def beyond(got, ref, bound):
    with np.errstate(invalid="ignore"):
        return (np.abs(got - ref) > bound).any()


def binned_bound(c, r):
    return bound_for(r.table, r.a, r.nt, r.recs, r.tmax, r.amax, r.ts, c.L, 1, P.LOG2_T, True)[0] + r.soft


def test_cases_tell_the_wrong_variants(big):
    """level features transposed; a clamp at +-14; the rescale weight missing from the table term; dec_l from another
    level: each moves an expected value beyond the bound the GPU test allows, in the case that is there for it"""
    c, fwd = big[6]
    assert not np.array_equal(fwd.lf.T.reshape(-1), fwd.lf.reshape(-1))  # [L][N] against [N][L]
    g = P.grad_with_silent_windows(c.n, seed=1)
    ref = P.backward_ref(c, fwd, g)
    wrong = P.backward_ref(c, fwd, g, dec_shift=1)
    assert beyond(wrong.table, ref.table, ref.atomic_bound()) and beyond(wrong.table, ref.table, binned_bound(c, ref))
    assert np.array_equal(wrong.ddec, ref.ddec)  # (the decoder gradient does not read the decoder)

    cs = P.saturation_case(2049, 6, seed=2)
    fs = P.forward_ref(cs)
    gs = P.saturation_grad(fs, seed=2)
    ref, wrong = P.backward_ref(cs, fs, gs), P.backward_ref(cs, fs, gs, clip=14.0)
    assert beyond(wrong.ddec, ref.ddec, ref.ddec_bound)
    assert beyond(wrong.table, ref.table, ref.atomic_bound()) and beyond(wrong.table, ref.table, binned_bound(cs, ref))

    cr = P.rescaled_case(1025, 6, seed=4)
    fr = P.forward_ref(cr)
    gr = P.grad_with_silent_windows(cr.n, seed=4)
    rt = P.rtol_rw(cr, fr)
    ref, wrong = P.backward_ref(cr, fr, gr, rw_rtol=rt), P.backward_ref(cr, fr, gr, use_rw=False, rw_rtol=rt)
    assert beyond(wrong.table, ref.table, ref.atomic_bound()) and beyond(wrong.table, ref.table, binned_bound(cr, ref))


def test_silent_windows_leave_entries_untouched(big):
    c, fwd = big[6]
    g = P.grad_with_silent_windows(c.n, seed=1)
    assert (g[64:128] == 0).all() and (g[192:256] == 0).all() and (g[32:64] == 0).all() and (g[:32] != 0).all()
    assert np.signbit(g[72:80]).all()
    ref = P.backward_ref(c, fwd, g)
    only_silent = ref.touched & (ref.nt == 0)
    assert only_silent.sum() >= 50 and (ref.table[only_silent] == 0).all()
    assert (ref.atomic_bound()[ref.nt > 0] > 0).all() and (ref.atomic_bound() < 1e-4 * np.maximum(ref.a, U)).all()
