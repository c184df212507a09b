"""CPU side of the scan, compaction and carry tests (tests/scan_refs.py): every precondition the GPU tests rely on, and the
evidence that their inputs can tell a wrong kernel from a right one.  Each scan is restated in numpy once as written and once
with its size-dependent branch broken (the carry between passes dropped, one block per thread forced, the strided loop cut
short).  The broken model must differ from the correct one wherever the new sizes enter that branch, and equals it at the
sizes the suite reached before -- which is why the gap went unnoticed.  At the exact boundary (nblk = 1024: one full pass,
one block per thread) the branch is not entered yet, so there the two models agree by construction; that case guards the
threshold itself and the last thread of a full pass."""
import numpy as np
import pytest

import occgrid_oracle as OO
import occgrid_update_restatement as UR
import scan_refs as SR


# ---- rows_scan_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SR.GRAD_T_NEW + (SR.GRAD_T_OLD,))
def test_rows_scan_model_and_the_dropped_carry(T):
    nblk = SR.grad_nblk(T)
    assert nblk == {262144: 1024, 262145: 1025, 262657: 1027, 4096: 16}[T]
    grad = SR.sparse_grad(T, 4, seed=T)
    nz = (grad != 0).any(-1)
    first = SR.GRAD_SCAN_WIDTH * SR.GRAD_ROWS_PER_BLOCK
    share = [[nz[l, :first].mean(), nz[l, first:].mean() if T > first + 256 else None] for l in range(2)]
    assert share[0][0] < 0.05 < 0.2 < share[1][0]  # the levels differ ...
    if T > first + 256:
        assert share[0][1] > 0.5 and share[1][1] < 0.15  # ... and so do the passes
    for l in range(2):
        counts = SR.block_counts(nz[l], SR.GRAD_ROWS_PER_BLOCK)
        assert len(counts) == nblk and nz[l, T - 1] and np.all(counts[-3:] > 0)
        good, broken = SR.rows_scan_model(counts), SR.rows_scan_model(counts, carry=False)
        np.testing.assert_array_equal(good, SR.exclusive_cumsum(counts))
        assert np.array_equal(good, broken) == (nblk <= SR.GRAD_SCAN_WIDTH)
        if nblk > SR.GRAD_SCAN_WIDTH:  # every block of the second pass is off by the first pass's total
            assert np.all(good[SR.GRAD_SCAN_WIDTH:] != broken[SR.GRAD_SCAN_WIDTH:])


def test_sparse_grad_rows_are_nonzero_in_some_feature_only():
    for F in (1, 4):
        g = SR.sparse_grad(SR.GRAD_T_OLD, F, seed=F)
        nz = (g != 0).any(-1)
        assert g.dtype == np.float32 and 0 < nz.sum() < nz.size
        if F > 1:
            assert ((g == 0) & nz[..., None]).any()  # a non-zero row with a zero in it


# ---- actor_pairs_scan_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SR.PAIRS_N_NEW + (SR.PAIRS_N_OLD,))
def test_hits_table_and_the_pairs_scan_with_one_block_per_thread(n):
    nblk = SR.pairs_nblk(n)
    assert nblk == {1048576: 1024, 1049600: 1025, 1049601: 1026, 70001: 69}[n]
    hits = SR.hits_table(n, seed=n)
    assert hits.dtype == np.int32 and hits.shape == (n, 8)
    # nrhip_actor_hits' layout: the hits in front, ascending and distinct, -1 behind
    k = (hits >= 0).sum(1)
    assert np.all((hits >= 0) == (np.arange(8)[None] < k[:, None])) and hits.max() < 32
    both = (hits[:, :-1] >= 0) & (hits[:, 1:] >= 0)
    assert np.all(hits[:, 1:][both] > hits[:, :-1][both])
    assert set(np.unique(k[:-1])) == {0, 1, 2, 3} and k[-1] == 8
    dens = [(k[:n // 2] > 0).mean(), (k[n // 2:] > 0).mean()]
    assert dens[0] > 0.1 and dens[1] < 0.03
    counts = SR.block_counts(hits >= 0, SR.PAIR_BLOCK * 8)
    b0, b1 = SR.empty_block_run(n)
    assert b1 - b0 >= 2 and not counts[b0:b1].any() and counts[b0 - 1] > 0 and counts[b1] > 0  # next to blocks that write
    good, total = SR.pairs_scan_model(counts)
    np.testing.assert_array_equal(good, SR.exclusive_cumsum(counts))
    assert total == counts.sum() == (hits >= 0).sum()
    broken, broken_total = SR.pairs_scan_model(counts, per=1)
    same = np.array_equal(good, broken) and total == broken_total
    assert same == (nblk <= SR.PAIR_SCAN_THREADS)
    if nblk > SR.PAIR_SCAN_THREADS:
        assert total != broken_total and np.all(good[SR.PAIR_SCAN_THREADS:] != broken[SR.PAIR_SCAN_THREADS:])
        # per = 2: an off-by-one in c0 = t * per would shift every thread's blocks; threads with c0 >= nblk own nothing
        assert -(-nblk // SR.PAIR_SCAN_THREADS) == 2 and (nblk + 1) // 2 < SR.PAIR_SCAN_THREADS


# ---- compact_scan_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [SR.OCC_RES_NEW, SR.OCC_RES_OLD])
@pytest.mark.parametrize("case", list(SR.CANDIDATE_CASES))
def test_candidate_cases_and_the_compact_scan_with_one_block_per_thread(case, res):
    c = SR.candidates_case(case, res)
    cells, n_blk, _ = SR.occ_sizes(res, c["L"])
    assert (res, n_blk) in ((65, 269), (32, 32))
    n, n_occ = c["n"], c["n_occ"]
    if case == "few_occupied":
        assert 0 < n_occ[0] <= n
    if case == "many_occupied":
        assert n_occ[0] > n
    if case == "two_levels":
        assert n_occ[0] > n >= n_occ[1] > 0
    assert (c["ids"] == -1).any() and (c["occs"] < 0).any()
    occs, binaries = c["occs"].reshape(c["L"], cells), c["binaries"].reshape(c["L"], cells)
    for l in range(c["L"]):
        visible = occs[l] >= 0
        sources = [visible, visible & binaries[l]] if c["warmup"] else \
            [visible[c["draws"]["cell_draws"][l]], visible & binaries[l]]
        for flags in sources:  # the flags of both compaction parts, as the count pass sees them
            counts = np.zeros(n_blk, np.int64)
            got = SR.block_counts(flags, SR.COMPACT_ITEMS)
            counts[:len(got)] = got  # (the draws fill only the first blocks: the rest count zero)
            good, total = SR.compact_scan_model(counts)
            np.testing.assert_array_equal(good, SR.exclusive_cumsum(counts))
            assert total == flags.sum()
            if len(flags) < cells:
                continue  # the n draws end before block 256: only the parts over all the cells reach the blocks behind it
            broken, broken_total = SR.compact_scan_model(counts, per=1)
            same = np.array_equal(good, broken) and total == broken_total
            assert same == (n_blk <= SR.OCC_SCAN_THREADS)  # the occupied cells span every block, in every case
            if not same:
                assert total != broken_total and np.all(good[SR.OCC_SCAN_THREADS:] != broken[SR.OCC_SCAN_THREADS:])
    if res == SR.OCC_RES_NEW:  # per = 2, threads from 135 on idle, a ragged last block of 193 cells
        assert -(-n_blk // 256) == 2 and -(-n_blk // 2) == 135 and cells % SR.COMPACT_ITEMS == 193


# ---- mean_final_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [SR.OCC_RES_NEW, SR.OCC_RES_OLD])
@pytest.mark.parametrize("regime", list(SR.EMA_OCC_THRE))
def test_ema_case_and_the_mean_over_the_first_256_partials_only(regime, res):
    L, occ_thre = 2, SR.EMA_OCC_THRE[regime]
    cells, _, n_part = SR.occ_sizes(res, L)
    assert (res, n_part) in ((65, 269), (32, 32))
    c = SR.ema_case(res, L, seed=71)
    ids, counts, vals, occs = c["ids"], c["counts"], c["vals"], c["occs"]
    assert ids.shape == (L, cells) and counts.tolist() == [cells, cells - 1000]
    assert np.all(vals * 1024 == np.round(vals * 1024)) and np.all((occs * 1024 == np.round(occs * 1024)))
    assert 0.15 < (occs < 0).mean() < 0.25
    touched = np.zeros((L, cells), bool)
    for l in range(L):
        touched[l, ids[l, :counts[l]]] = True
        assert len(np.unique(ids[l, :counts[l]])) < 0.7 * counts[l]  # duplicates
    assert 0.3 < (~touched).mean() < 0.45  # and cells no candidate names
    new = UR.ema(occs, res, ids, counts, vals, SR.EMA_DECAY)
    assert (new != occs).any() and np.array_equal(new[occs < 0], occs[occs < 0])
    want_b, want_thre, want_mean = UR.threshold(new, occ_thre)
    print(f"res {res}: mean {want_mean:.6g}, thre {want_thre:.6g}, nearest value {UR.threshold_gap(new, want_thre):.3g} (relative)")
    if res == SR.OCC_RES_NEW:  # what the GPU test relies on
        assert (want_mean > occ_thre) == (regime == "mean_above_occ_thre")
        assert UR.threshold_gap(new, want_thre) > 1e-3
    assert 0 < want_b.sum() < want_b.size
    psum, pcnt = SR.visible_partials(new)
    assert len(psum) == n_part
    thre, mean = SR.mean_final_model(psum, pcnt, occ_thre)
    assert abs(mean - want_mean) <= 1e-12 * want_mean and thre == want_thre
    bad_thre, bad_mean = SR.mean_final_model(psum, pcnt, occ_thre, strided=False)
    if n_part <= SR.OCC_SCAN_THREADS:
        assert bad_thre == thre and bad_mean == mean
    else:  # the cut-short loop moves the threshold across cells' values: the binaries differ
        assert bad_thre < thre and ((new > bad_thre) != want_b).sum() > 1000


@pytest.mark.parametrize("occ_thre", [1e-3, 1e-2])
def test_shell_scenario_at_the_default_resolution(occ_thre):
    """res 128, one level: the restatement's mean lies above both thresholds at every step (so thre = occ_thre), and no
    visible cell's value lies within 1e-3, relative, of the threshold"""
    cells, n_blk, n_part = SR.occ_sizes(128, 1)
    assert (n_blk, n_part) == (2048, 1024) and -(-n_blk // 256) == 8
    for step, d, out in SR.shell_run_default(occ_thre):
        gap = UR.threshold_gap(out["occs"], out["thre"])
        print(f"step {step}: mean {out['mean']:.6g} thre {out['thre']:.6g} nearest value {gap:.3g} (relative)")
        assert gap > 1e-3
        assert out["mean"] > occ_thre and out["thre"] == np.float32(occ_thre)
        np.testing.assert_array_equal(out["binaries"].reshape(-1), out["occs"] > out["thre"])
        assert 0 < out["binaries"].sum() < cells


# ---- packed_visibility_kernel ----------------------------------------------------------------------------------------------
def test_exact_visibility_rays_cross_eps_where_they_were_designed_to():
    seg, a = SR.vis_segments(), SR.vis_exact_alphas()
    assert len(seg) == 14 and seg[-1] == 2153 == len(a) and a.dtype == np.float32
    assert set(np.unique(a)) == {0.0, 0.5, 0.75}
    eps = SR.VIS_EXACT_EPS
    T = SR.transmittance64(a, seg)
    assert np.all(np.log2(T) == np.round(np.log2(T)))  # powers of two: fp32 and float64 agree on every comparison
    assert SR.first_below(T, seg, eps) == SR.VIS_EXACT_CROSS
    touches = tuple(bool((T[b:e] == eps).any()) for b, e in zip(seg[:-1], seg[1:]))
    assert touches == SR.VIS_EXACT_TOUCH
    # where each crossing falls: inside chunk 0; at samples 63, 64 and 65; inside chunk 2; inside a ragged last chunk; never
    cross = dict(zip(SR.VIS_LENGTHS[1:], SR.VIS_EXACT_CROSS[1:]))
    assert (cross[63], cross[64], cross[65], cross[128], cross[129], cross[191]) == (30, 63, 64, 65, 64, 150)
    assert 2 * 64 < cross[191] < 191 and 191 % 64 and 10 * 64 < cross[700] < 700 and 700 % 64 and cross[512] is None
    # the carry out of chunk 0 equals eps exactly in the ray that crosses at 65: kept going, sample 64 kept
    b = seg[5]
    assert SR.VIS_LENGTHS[5] == 128 and T[b + 64] == eps and T[b + 65] < eps
    # the kernel stops behind chunk ceil(c / 64) - 1, the first whose outgoing carry T[64 (j + 1)] lies below eps; the chunks
    # behind it are zero-filled: one (65), two (129), four (300), none (128)
    behind = {n: -(-n // 64) - -(-c // 64) for n, c in cross.items() if c}
    assert (behind[65], behind[129], behind[300], behind[128]) == (1, 2, 4, 0)
    for thre in SR.VIS_ALPHA_THRES:
        want, _ = SR.visibility64(a, seg, eps, thre)
        np.testing.assert_array_equal(want, OO.packed_visibility_from_alpha(a, seg, eps, thre))
        np.testing.assert_array_equal(want, SR.visibility_model(a, seg, eps, thre))
        assert (want != SR.visibility_model(a, seg, eps, thre, carry=False)).any()
        for (b, e), c in zip(zip(seg[:-1], seg[1:]), SR.VIS_EXACT_CROSS):  # something is kept right up to each crossing
            if c is not None and thre <= 0.5:
                assert want[b + c - 1] and not want[b + c:e].any()
    kept = [SR.visibility64(a, seg, eps, t)[0].sum() for t in SR.VIS_ALPHA_THRES]
    assert kept[0] > kept[1] > kept[2] > 0  # each alpha_thre decides something


def test_the_suites_earlier_visibility_input_could_not_see_a_dropped_carry():
    """constant alpha 0.5, 35 samples per ray, eps 1e-2: one chunk per ray"""
    seg = SR.vis_segments([35] * 64)
    a = np.full(seg[-1], 0.5, np.float32)
    want = OO.packed_visibility_from_alpha(a, seg, 1e-2, 0.0)
    np.testing.assert_array_equal(want, SR.visibility_model(a, seg, 1e-2, 0.0))
    np.testing.assert_array_equal(want, SR.visibility_model(a, seg, 1e-2, 0.0, carry=False))


def test_generic_visibility_band_and_crossings():
    seg, a = SR.vis_segments(), SR.vis_generic_alphas()
    eps, thre = SR.VIS_GENERIC_EPS, SR.VIS_GENERIC_ALPHA_THRE
    assert a.dtype == np.float32 and a.min() >= 0 and a.max() <= 0.05
    want, T = SR.visibility64(a, seg, eps, thre)
    left_out = np.abs(T - eps) <= SR.VIS_BAND * eps
    print(f"{left_out.sum()} of {len(a)} samples within {SR.VIS_BAND} (relative) of eps")
    assert left_out.mean() <= SR.VIS_MAX_LEFT_OUT
    # fewer than 1024 roundings of 2^-24 each stay inside the band
    assert max(SR.VIS_LENGTHS) < 1024 and 1024 * 2.0 ** -24 < SR.VIS_BAND
    cross = SR.first_below(T, seg, eps)
    assert sum(c is not None and c >= 64 for c in cross) >= 3
    assert not np.any(a == np.float32(thre))  # no alpha sits on the threshold's own rounding
    sure = ~left_out
    np.testing.assert_array_equal(want[sure], OO.packed_visibility_from_alpha(a, seg, eps, thre)[sure])
    np.testing.assert_array_equal(want[sure], SR.visibility_model(a, seg, eps, thre)[sure])
    assert (want != SR.visibility_model(a, seg, eps, thre, carry=False))[sure].sum() > 100
    assert 0.2 < want.mean() < 0.8 and 0.2 < (a >= np.float32(thre)).mean() < 0.8
