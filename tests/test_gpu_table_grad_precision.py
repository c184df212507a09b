"""The binned table gradient (csrc/encode_bwd_binned.hip) entry by entry, at a trained scene's gradient magnitudes.

`reduce` adds a slice's records in 64-bit fixed point with ONE scale per (level, slice): sh = 61 - hb - (e + 1), where
2^e <= vmax < 2^(e+1) is the level's largest |record value| and hb = (PAIR ? 33 : 32) - clz(records in the slice).  Every
record is rounded to the quantum q = 2^-sh once; the integer sum is exact; the result is rounded to fp32 once.  So for an
entry with reference sum g, sum of |terms| a and n terms:

    |got - g| <= n q / 2 + 32 u a + u |g|            (u = 2^-24)

n q / 2: n roundings to the quantum.  32 u a: the record values are fp32 products (corner weight times incoming gradient,
a few roundings each) and runs of up to 16 equal keys are merged in fp32 before they become records.  u |g|: the final
rounding.  The test recomputes q from upper bounds on the kernel's vmax and record count (a record holds at most 16 merged
terms; records <= terms), so q here is >= the kernel's.  A whole-table rel-L2 is dominated by the largest entries; this
bound holds for each of them, down to entries of 1e-14 in a level whose largest gradient is 1e2."""
import numpy as np
import pytest
import torch

import neurad_oracle as O
import synth
from gpu_util import dev, host64_via32
from gpu_util import ops  # noqa: F401  (fixture)
from table_grad_refs import U, bound_for, check_entries, log2_slice, quantum, reference  # noqa: F401

pytestmark = pytest.mark.gpu

LAYOUT = (4, 1, 14, 16, 1024)  # (L, F, log2 T, min_res, max_res): proposal-grid-like, several slices per level
N = (1 << 16) + 37


def sharp_gradients(n, L, F, seed, scale):
    """incoming gradients of a trained scene: transmittance T in [1e-12, 1] times O(1e-2 .. 1e2) -> 1e-14 .. 1e2 in every
    level; a tenth of the samples silent (behind a surface); times a GradScaler scale"""
    T = 10.0 ** synth.uniform((n, 1), -12.0, 0.0, seed)
    mag = 10.0 ** synth.uniform((n, L * F), -2.0, 2.0, seed + 1)
    g = (synth.normal((n, L * F), seed + 2) * mag * T * scale).astype(np.float32)
    g[synth.uniform((n,), 0, 1, seed + 3) < 0.1] = 0.0
    return g


def positions(n, seed):
    x = synth.uniform((n, 3), 0.0, 1.0, seed)
    x[: n // 8] = np.float32(0.5) + (x[: n // 8] - np.float32(0.5)) * np.float32(1e-3)  # a hot spot: long runs, big a
    return x


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 16, 2.0 ** 24], ids=["unscaled", "scale2^16", "scale2^24"])
@pytest.mark.parametrize("pairs", ["all", "none"])
def test_hashgrid_bwd_binned_per_entry_bound(ops, monkeypatch, switches, pairs, scale):
    """hashgrid_bwd through the radix partition, x-pair records on and off (NRHIP_BIN_PAIRS, F = 1), gradients spanning
    1e-14 .. 1e2 in each level, unscaled and under GradScaler scales: every entry within the design's bound; entries far
    above the quantum to 1e-6; tiny entries (|g| < n q) that come back 0 or with the wrong sign are counted and reported"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    monkeypatch.setattr(ops, "_FORCE_ATOMIC_SCATTER", False)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    L, F, lg, mn, mx = LAYOUT
    x = positions(N, 3)
    go = sharp_gradients(N, L, F, 11, scale)
    spec = ops.GridSpec(L, F, lg, mn, mx)
    got = host64_via32(ops.hashgrid_bwd(spec, None, dev(x), dev(go))).reshape(-1)
    ref, a, n, recs, tmax, amax, ts = reference(x, go, L, F, lg, mn, mx)
    pair = pairs == "all"
    bnd, q = bound_for(ref, a, n, recs, tmax, amax, ts, L, F, lg, pair)
    assert np.isfinite(got).all()
    check_entries(got, ref, bnd, f"pairs={pairs} scale={scale}")
    assert (got[n == 0] == 0).all()  # untouched entries are exactly 0
    big = np.abs(ref) > 2.0 ** 20 * n * q  # n q / 2 < 1e-6 |g| there
    assert big.sum() > 100
    assert (np.abs(got - ref)[big] <= 1e-6 * np.abs(ref[big]) + 32 * U * a[big]).all()
    tiny = (ref != 0) & (np.abs(ref) < n * q)
    lost = tiny & ((got == 0) | (np.sign(got) != np.sign(ref)))
    touched = int((n > 0).sum())
    print(f"\n[pairs={pairs} scale={scale:g}] entries {touched}, tiny (0 < |g| < n q) {int(tiny.sum())}, "
          f"of those zero or wrong sign {int(lost.sum())}; q per level {[float(v) for v in q.reshape(L, -1).max(1)]}")
    # only tiny entries may come back 0 or flipped (the bound says so), and at 16 decades of gradient per level they are
    # ~0.04 % of the touched entries here: more than 0.1 % would mean the quantum grew
    assert not ((ref != 0) & ~tiny & ((got == 0) | (np.sign(got) != np.sign(ref)))).any()
    assert lost.sum() <= 1e-3 * touched, (int(lost.sum()), touched)


def exact_case(L, lg, mn, mx, n0, seed):
    """positions whose records are known exactly: no two samples share a (level, corner slot) key -- distinct cells and no
    hash collision -- so `emit` merges nothing (a merge needs the same key in neighbouring lanes), every corner term is one
    record, and each slice's record count and each level's vmax are the reference's own.  Level l's gradients are scaled by
    10^(-3 l): a `reduce` that took another level's scale would be off by 1000x."""
    scal = O.hash_scalings(L, mn, mx)
    x = synth.uniform((n0, 3), 0.0, 1.0, seed)
    idx, _ = O.hashgrid_corner_indices(x, scal, 1 << lg)
    keep = np.ones(n0, bool)
    for c in idx.reshape(n0, -1).T:  # keep a sample only where it is the first to use its key in every column
        first = np.zeros(n0, bool)
        first[np.unique(c, return_index=True)[1]] = True
        keep &= first
    T = 10.0 ** synth.uniform((n0, 1), -12.0, 0.0, seed + 1)
    g = synth.normal((n0, L), seed + 2) * 10.0 ** synth.uniform((n0, L), -2.0, 2.0, seed + 3) * T
    g = (g * 10.0 ** (-3.0 * np.arange(L))[None, :]).astype(np.float32)
    return x, g, keep, idx


def slice_counts(idx, rows, L, lg, ts):
    ent = idx[rows] - (np.arange(L) * (1 << lg))[None, :, None]
    sl = (np.arange(L)[None, :, None] << (lg - ts)) + (ent >> ts)
    return sl, np.bincount(sl.reshape(-1), minlength=L << (lg - ts))


def test_binned_quantum_is_exactly_the_designs(ops, monkeypatch, switches):
    """The fixed-point quantum itself, not an upper bound on it: with every record known (exact_case), q = 2^-sh follows
    from the kernel's formula with the level's true vmax and the slice's true record count.  One level-0 slice is trimmed
    to exactly 2^k - 2 records (hb = k) and one level-1 slice to exactly 2^k' (hb = k' + 1).  Each entry must satisfy
    |got - g| <= n q / 2 + 8 u a + 2 u |g| (one quantum rounding per record, the fp32 corner-weight product, the final
    rounding), and on entries of one record where n q / 2 dominates the rest, the largest error must use more than 3/4 of
    q / 2: the quantum is neither coarser (an hb one bit high, truncation for __float2ll_rn, another level's vmax) nor
    finer (an hb one bit low) than the design's -- in every slice and in the two power-of-two slices."""
    switches.set("NRHIP_BIN_PAIRS", "none")  # one corner term per record
    monkeypatch.setattr(ops, "_FORCE_ATOMIC_SCATTER", False)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    L, F, lg, mn, mx = 2, 1, 19, 512, 1024
    x, go, keep, idx = exact_case(L, lg, mn, mx, 12000, 41)
    ts = log2_slice(L, F, lg)
    rows = np.flatnonzero(keep)
    sl, cnt = slice_counts(idx, rows, L, lg, ts)
    ns = 1 << (lg - ts)
    targets = []
    for lvl, want_pow2 in ((0, False), (1, True)):  # trim one slice per level by dropping samples that send it one record
        s = lvl * ns + int(np.argmax(cnt[lvl * ns:(lvl + 1) * ns]))
        k = int(cnt[s]).bit_length() - 1
        goal = (1 << k) if want_pow2 else (1 << k) - 2  # (a slice's count is even: x-pairs never straddle a slice here)
        m = (sl == s).sum((1, 2)) * ~np.isin(sl, targets).any((1, 2))  # records each sample sends to slice s
        left, drop = int(cnt[s]) - goal, []
        for i in np.argsort(-m, kind="stable"):  # greedy, largest first: ends on samples that send one record
            if 0 < m[i] <= left:
                drop.append(i)
                left -= int(m[i])
        rows = np.delete(rows, drop)
        sl, cnt = slice_counts(idx, rows, L, lg, ts)
        assert cnt[s] == goal
        targets.append(s)
    xs, gs = x[rows], go[rows]
    spec = ops.GridSpec(L, F, lg, mn, mx)
    got = host64_via32(ops.hashgrid_bwd(spec, None, dev(xs), dev(gs))).reshape(-1)
    ref, a, n, recs, tmax, amax, ts2 = reference(xs, gs, L, F, lg, mn, mx)
    assert ts2 == ts and np.array_equal(recs, cnt)
    # vmax: the largest fp32 record of the level.  The fp32 product is within 8u of the float64 term; where that straddles a
    # power of two the larger exponent is taken (q then allows 2x in that level only)
    e = np.maximum(np.frexp(tmax * (1 - 8 * U))[1], np.frexp(tmax * (1 + 8 * U))[1]) - 1
    hb = np.array([int(c).bit_length() for c in cnt])  # PAIR = 0: 32 - clz(cnt)
    sh = 61 - hb - (np.repeat(e, ns) + 1)
    q = np.repeat(np.ldexp(1.0, -sh), 1 << ts)
    rest = 8 * U * a + 2 * U * np.abs(ref)
    check_entries(got, ref, n * q / 2 + rest, "exact quantum")
    one = (n == 1) & (q / 2 > 20 * rest)
    ratio = np.abs(got - ref) / (q / 2)
    ent_slice = np.repeat(np.arange(L * ns), 1 << ts)
    for lvl in range(L):
        m = one & (ent_slice // ns == lvl)
        assert m.sum() > 500, (lvl, int(m.sum()))
        assert ratio[m].max() > 0.75, f"level {lvl}: the quantum is finer than the design's ({ratio[m].max():.3f})"
    for t in targets:
        m = one & (ent_slice == t)
        assert m.sum() >= 20 and ratio[m].max() > 0.75, (t, int(cnt[t]), int(m.sum()), float(ratio[m].max(initial=0)))


def test_hashgrid_adam_step_on_binned_gradient(ops, monkeypatch):
    """One HashGridAdam step (eps = 1e-15, the table optimizer's) on the binned gradient against torch.optim.Adam in float64
    on the exact gradient: a first Adam step moves an entry by ~ lr sign(g) however small g is, so an entry the fixed point
    rounds to 0 or flips moves by lr the wrong way.  Every entry whose update differs by more than lr / 2 must be one the
    bound allows to be that far off (error bound >= |g| / 2); the count is reported."""
    from neurad_studio_amd.optim import HashGridAdam

    monkeypatch.setattr(ops, "_FORCE_ATOMIC_SCATTER", False)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    L, F, lg, mn, mx = LAYOUT
    x = positions(N, 5)
    go = sharp_gradients(N, L, F, 21, 1.0)
    spec = ops.GridSpec(L, F, lg, mn, mx)
    got = ops.hashgrid_bwd(spec, None, dev(x), dev(go))
    ref, a, n, recs, tmax, amax, ts = reference(x, go, L, F, lg, mn, mx)
    bnd, q = bound_for(ref, a, n, recs, tmax, amax, ts, L, F, lg, ops_pairs_default(F))
    lr = 1e-2
    table = dev(synth.hash_table(L << lg, F, seed=7, scale=1e-3))
    p = torch.nn.Parameter(table.clone())
    opt = HashGridAdam([p], lr=lr, eps=1e-15)
    p.grad = got
    opt.step()
    upd = host64_via32(p.detach() - table).reshape(-1)
    p64 = torch.nn.Parameter(torch.tensor(host64_via32(table)))
    opt64 = torch.optim.Adam([p64], lr=lr, eps=1e-15)
    p64.grad = torch.tensor(ref.reshape(-1, F))
    opt64.step()
    upd64 = (p64.detach() - torch.tensor(host64_via32(table))).numpy().reshape(-1)
    off = np.abs(upd - upd64) > lr / 2
    explained = bnd >= np.abs(ref) / 2
    print(f"\n[adam] entries with a gradient {int((n > 0).sum())}, updates off by > lr/2: {int(off.sum())} "
          f"({int((off & (ref != 0)).sum())} with g != 0), |g| of those <= {float(np.abs(ref[off]).max(initial=0)):.3g}")
    assert not (off & ~explained).any(), f"{int((off & ~explained).sum())} Adam updates off beyond the fixed-point bound"


def ops_pairs_default(F):
    return F == 1  # use_pairs(): x-pair records at F = 1 unless NRHIP_BIN_PAIRS says otherwise


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 24], ids=["unscaled", "scale2^24"])
def test_multi_grid_binned_per_entry_bound_and_fp16_overflow(ops, monkeypatch, scale):
    """hashgrid_multi_bwd (the actor grids) through the partition, fp32 and fp16 output.  fp16: every entry is the fp16
    rounding of a value within the bound, and an entry whose value rounds beyond fp16's range (|g| >= 65520) comes back
    as +-inf -- never finite -- so that the non-finite check / GradScaler skips the step"""
    monkeypatch.setattr(ops, "_FORCE_ATOMIC_SCATTER", False)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    L, F, lg, mn, mx = 4, 2, 12, 16, 512
    n_grids = 2
    x = positions(N, 9)
    go = sharp_gradients(N, L, F, 31, scale)
    gid = (synth.uniform((N,), 0, 1, 33) < 0.3).astype(np.int32)  # 30 % of the samples in grid 1
    spec = ops.GridSpec(L, F, lg, mn, mx)
    out32 = ops.hashgrid_multi_bwd(spec, n_grids, dev(gid, torch.int32), dev(x), dev(go))
    out16 = ops.hashgrid_multi_bwd(spec, n_grids, dev(gid, torch.int32), dev(x), dev(go), out_dtype=torch.float16)
    refs = [reference(x[gid == k], go[gid == k], L, F, lg, mn, mx, n_slots=n_grids) for k in range(n_grids)]
    tmax = np.maximum(refs[0][4], refs[1][4])  # vmax is per level over all grids' records
    amax = np.maximum(refs[0][5], refs[1][5])
    for k in range(n_grids):
        ref, a, n, recs, _, _, ts = refs[k]
        bnd, q = bound_for(ref, a, n, recs, tmax, amax, ts, L, F, lg, ops_pairs_default(F))
        g32 = host64_via32(out32[k]).reshape(-1)
        assert out16[k].dtype == torch.float16
        g16 = host64_via32(out16[k]).reshape(-1)
        assert np.isfinite(g32).all()  # (|g| <= 1e2 * 2^24 * n: far inside fp32's range at either scale)
        check_entries(g32, ref, bnd, f"multi grid {k} fp32")
        fin = np.abs(ref) + bnd < 65504  # surely inside fp16's range
        ovf = np.abs(ref) - bnd >= 65520  # surely beyond it
        b16 = bnd + 2.0 ** -11 * (np.abs(ref) + bnd) + 2.0 ** -25  # + fp16's rounding (its subnormal half-spacing)
        check_entries(g16[fin], ref[fin], b16[fin], f"multi grid {k} fp16")
        assert np.isfinite(g16[fin]).all()
        if scale > 1:
            assert ovf.sum() > 10
            assert np.isinf(g16[ovf]).all() and (np.sign(g16[ovf]) == np.sign(ref[ovf])).all(), \
                f"grid {k}: {int((~np.isinf(g16[ovf])).sum())} fp16 entries beyond 65520 came back finite"


@pytest.mark.parametrize("pairs", ["all", "none"])
def test_binned_poisoning_hits_exactly_the_poisoned_entries(ops, monkeypatch, switches, pairs):
    """Inf / NaN in an incoming gradient poisons (NaN) exactly the entries its terms go to -- all 8 corners of that sample,
    level and feature, a zero corner weight included (0 * inf is NaN in the reference too) -- and nothing else.  Three of
    the four poisoned (sample, level) pairs have x-pairs whose floor and ceil corners lie in two different slices: with
    pairs on, `emit` sends those as two records (the floor values with a zeroed ceil half, and the ceil values into the
    other slice), so the poison bit has to land on the other slice's accumulator too."""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    monkeypatch.setattr(ops, "_FORCE_ATOMIC_SCATTER", False)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    L, F, lg, mn, mx = 4, 1, 14, 256, 4096
    n = 40000
    rng = np.random.default_rng(3)
    x = rng.uniform(0.02, 0.98, (n, 3)).astype(np.float32)
    scal = O.hash_scalings(L, mn, mx)
    for l in range(L):  # rows l + 8j: floor(x * scale_l) = 2^k - 1, k >= 9 (capped below the resolution)
        rows = np.arange(l, n, 2 * L)
        cell = np.minimum((1 << rng.integers(9, 12, rows.size)) - 1, int(scal[l]) - 2)
        x[rows, 0] = ((cell + rng.uniform(0.1, 0.9, rows.size)) / scal[l]).astype(np.float32)
    idx, _ = O.hashgrid_corner_indices(x, scal, 1 << lg)
    ts = log2_slice(L, F, lg)
    ent = idx - (np.arange(L) * (1 << lg))[None, :, None]
    # (floor x, ceil x) corner slots of the reference order, as kPairF / kPairC in encode_bwd_binned.hip
    straddles = ((ent[:, :, [3, 2, 7, 6]] >> ts) != (ent[:, :, [0, 1, 4, 5]] >> ts)).any(-1)  # [n, L]
    r3 = [r for r in range(3, n, 2 * L) if straddles[r, 3]][:2]
    r2 = [r for r in range(2, n, 2 * L) if straddles[r, 2]][:1]
    bad = [(r3[0], 3, np.inf), (r3[1], 3, np.nan), (r2[0], 2, -np.inf), (123, 0, np.nan)]
    assert [bool(straddles[r, c]) for r, c, _ in bad] == [True, True, True, False]
    go = synth.normal((n, L * F), 17)
    for r, c, v in bad:
        go[r, c] = v
    spec = ops.GridSpec(L, F, lg, mn, mx)
    got = host64_via32(ops.hashgrid_bwd(spec, None, dev(x), dev(go))).reshape(-1)
    want = np.zeros(got.shape, bool)
    for r, c, _ in bad:
        l, j = divmod(c, F)
        want[idx[r, l] * F + j] = True
    assert (~np.isfinite(got) == want).all(), (np.flatnonzero(~np.isfinite(got) & ~want)[:5],
                                               np.flatnonzero(want & np.isfinite(got))[:5])
