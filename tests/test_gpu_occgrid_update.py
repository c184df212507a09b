"""Occupancy-grid maintenance on the GPU against its CPU restatement (tests/occgrid_update_restatement.py): candidates,
positions, EMA, threshold, gating and state, the multi-level march, invisible cells, the route end to end, density_fn.
The rule is modelled on nerfacc 0.5 (csrc/occgrid_update.h); nerfacc is un-vendored, so parity with nerfacc itself is
unpinned -- what is pinned is the stated rule.  Discrete decisions are compared exactly; where a comparison of rounded
numbers decides (a midpoint on a cell face, a projection on an image edge) the float64 restatement names the cases to leave
out, and their share is bounded."""
import numpy as np
import pytest
import torch

import occgrid_update_restatement as UR
import scan_refs as SR
import synth
from conftest import rel_l2
from gpu_util import cuda, host

pytestmark = pytest.mark.gpu

TIGHT = 2e-5  # tests/test_gpu_packed.py
UNIT = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev_draws(d, warmup):
    return dict(cell_draws=None if warmup else cuda(d["cell_draws"]), sel_draws=None if warmup else cuda(d["sel_draws"]),
                jitter=cuda(d["jitter"]))


def shell_occ_torch(p):
    x = p.double()
    r = torch.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])
    return (torch.floor(torch.clamp(1.5 - r, 0.0, 1.0) * 8.0) / 256.0).float()


def random_state(res, L, seed, p_invisible=0.2, p_occupied=0.5):
    rng = np.random.default_rng(seed)
    occs = rng.random(L * res ** 3).astype(np.float32)
    occs[rng.random(occs.shape) < p_invisible] = -1.0
    binaries = (rng.random((L, res, res, res)) < np.reshape(p_occupied, (-1, 1, 1, 1)))
    return occs, binaries


# ---- candidates ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["warmup_with_invisible", "few_occupied", "many_occupied", "two_levels"])
def test_candidates_equal_the_restatement(case):
    from neurad_studio_amd import ops

    res = 16
    L = 2 if case == "two_levels" else 1
    warmup = case == "warmup_with_invisible"
    p_occ = {"warmup_with_invisible": 0.5, "few_occupied": 0.1, "many_occupied": 0.6, "two_levels": [0.6, 0.1]}[case]
    occs, binaries = random_state(res, L, 11, p_occupied=p_occ)
    d = UR.draws(res, L, warmup, 12)
    n, cap = UR.capacity(res, warmup)
    want_ids, want_counts = UR.candidates(occs, binaries, res, L, warmup, None, d["cell_draws"], d["sel_draws"])
    n_occ = (binaries.reshape(L, -1) & (occs.reshape(L, -1) >= 0)).sum(1)
    if case == "few_occupied":
        assert 0 < n_occ[0] <= n
    if case == "many_occupied":
        assert n_occ[0] > n
    if case == "two_levels":
        assert n_occ[0] > n >= n_occ[1] > 0
    grid = ops.OccGridSpec(torch.tensor(UNIT), cuda(binaries))
    ids, counts, pos = ops.occgrid_update_candidates(grid, cuda(occs), warmup, **dev_draws(d, warmup))
    assert ids.shape == (L, cap) and pos.shape == (L * cap, 3)
    np.testing.assert_array_equal(host(counts), want_counts)
    np.testing.assert_array_equal(host(ids), want_ids)
    assert (want_ids == -1).any() and (occs < 0).any()


@pytest.mark.parametrize("box", [UNIT, [-1.3, -2.1, 0.2, 3.3, 1.7, 2.9]], ids=["power_of_two", "generic"])
def test_positions_lie_in_their_cells(box):
    """Each position is within 4 ulp (of the box's largest coordinate magnitude) of the restatement: three fp32 roundings of
    at most half an ulp each, doubled.  Each lies in its cell's closed box, with no slack: against the real faces where they
    are fp32 numbers (the power-of-two box), and for any box against the faces in the update's own fp32 arithmetic, which
    every position must respect because each step of the formula is monotone (those faces are within the same 4 ulp of the
    real ones)."""
    from neurad_studio_amd import ops

    res, L = 16, 2
    occs, binaries = random_state(res, L, 21)
    d = UR.draws(res, L, False, 22)
    d["jitter"][0, :8] = np.float32(1.0 - 2.0 ** -24)  # the largest jitter there is
    d["jitter"][0, 8:16] = 0.0
    aabbs = UR.level_aabbs(box, L)
    grid = ops.OccGridSpec(torch.from_numpy(aabbs), cuda(binaries))
    ids, counts, pos = ops.occgrid_update_candidates(grid, cuda(occs), False, **dev_draws(d, False))
    ids, pos = host(ids), host(pos).reshape(L, -1, 3)
    want32, want64 = UR.positions(aabbs, res, ids, d["jitter"]), UR.positions(aabbs, res, ids, d["jitter"], np.float64)
    lo, hi = UR.cell_boxes(aabbs, res, ids)
    flo, fhi = UR.cell_faces_f32(aabbs, res, ids)
    for l in range(L):
        ulp = float(np.spacing(np.float32(np.abs(aabbs[l]).max())))
        ok = ids[l] >= 0
        err = np.abs(pos[l].astype(np.float64) - want64[l])
        print(f"level {l}: max |p - float64 restatement| = {err[ok].max() / ulp:.2f} ulp; differs from the fp32 restatement on "
              f"{(bits(pos[l]) != bits(want32[l])).sum()} coordinates")
        assert err.max() <= 4 * ulp
        if box is UNIT:  # the faces are fp32 numbers: the real box, exactly
            assert np.all(pos[l][ok] >= lo[l][ok]) and np.all(pos[l][ok] <= hi[l][ok])
        assert np.all(pos[l][ok] >= flo[l][ok]) and np.all(pos[l][ok] <= fhi[l][ok])  # fp32 faces: exactly, any box
        assert np.all(np.abs(flo[l] - lo[l]) <= 4 * ulp) and np.all(np.abs(fhi[l] - hi[l]) <= 4 * ulp)
        centre = ((aabbs[l, :3] + aabbs[l, 3:]) * np.float32(0.5))
        np.testing.assert_array_equal(pos[l][~ok], np.broadcast_to(centre, pos[l][~ok].shape))


# ---- EMA -------------------------------------------------------------------------------------------------------------------
def test_ema_takes_the_max_over_duplicates_and_decays_once():
    from neurad_studio_amd import ops

    res, L, decay = 8, 2, 0.95
    cells, cap = res ** 3, 256
    occs, binaries = random_state(res, L, 31)
    occs[[5, 6, 7, 8, cells + 3]] = [0.5, 0.25, 0.0, -1.0, 0.75]  # visible, visible, zero, INVISIBLE, level 1
    rng = np.random.default_rng(32)
    visible = [np.nonzero(occs[l * cells:(l + 1) * cells] >= 0)[0] for l in range(L)]
    ids = np.full((L, cap), -1, np.int32)
    vals = rng.normal(0, 1, (L, cap)).astype(np.float32)
    counts = np.array([200, 120], np.int32)
    for l in range(L):
        ids[l, :counts[l]] = rng.choice(visible[l][visible[l] > 16], counts[l])  # random cells, with repeats
    # explicit duplicates, any order: the max wins, mixed signs, all negative, below the decayed value, an invisible cell
    ids[0, :12] = [5, 6, 5, 7, 5, 6, 7, 8, 8, 6, 7, 5]
    vals[0, :12] = [0.1, -0.5, 0.9, -0.3, 0.6, -0.25, -0.2, 5.0, 7.0, -1.5, -0.1, 0.9]
    ids[1, :4] = [3, 3, 3, 3]
    vals[1, :4] = [0.1, 0.2, 0.3, 0.05]  # all below 0.75 * 0.95
    ids[0, 12:16] = [10, 10, 11, 11]  # NaN counts as no candidate: cell 10 takes its other value, cell 11 is untouched
    vals[0, 12:16] = [np.nan, 0.8, np.nan, -np.nan]
    occs[[10, 11]] = [0.5, 0.5]
    ids[0, 210:214] = [5, 6, 7, 9]  # behind the count: ignored whatever they hold
    vals[0, 210:214] = 100.0
    grid = ops.OccGridSpec(torch.tensor(UNIT), cuda(binaries))
    got = cuda(occs)
    ops.occgrid_update_apply(grid, got, cuda(ids), cuda(counts), cuda(vals), decay, 1e-2)
    got = host(got)
    want = occs.copy()
    for l in range(L):  # written out cell by cell
        for c in np.unique(ids[l, :counts[l]]):
            i = l * cells + c
            v = vals[l, :counts[l]][ids[l, :counts[l]] == c]
            if occs[i] >= 0 and not np.isnan(v).all():
                want[i] = max(np.float32(occs[i] * np.float32(decay)), np.nanmax(v))
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(got), bits(UR.ema(occs, res, ids, counts, vals, decay)))
    assert got[5] == np.float32(0.9) and got[6] == np.float32(0.25 * np.float32(decay)) and got[7] == 0.0
    assert got[10] == np.float32(0.8) and got[11] == np.float32(0.5)
    assert got[8] == -1.0 and got[cells + 3] == np.float32(0.75 * np.float32(decay))
    touched = np.zeros(L * cells, bool)
    for l in range(L):
        touched[l * cells + ids[l, :counts[l]]] = True
    assert (~touched).sum() > 100
    np.testing.assert_array_equal(bits(got[~touched]), bits(occs[~touched]))  # untouched cells keep their bits
    np.testing.assert_array_equal(got[occs < 0], -1.0)                        # invisible cells are never written
    b, thre, _ = UR.threshold(want, 1e-2)
    np.testing.assert_array_equal(host(grid.binaries).reshape(-1), b)


# ---- threshold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occ_thre", [1e-3, 1e-2], ids=["mean_above_occ_thre", "mean_below_occ_thre"])
def test_threshold_on_the_quantised_shell(occ_thre):
    """binaries equal the restatement's on EVERY cell, over two warm-up and two later updates, res 32, two levels.
    Precondition (asserted): no visible cell's value lies within 1e-3, relative, of the restatement's threshold."""
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    est = OccGridEstimator(UNIT, resolution=32, levels=2)
    for step, d, want in UR.shell_run(occ_thre):
        gap = UR.threshold_gap(want["occs"], want["thre"])
        assert gap > 1e-3
        assert (want["mean"] > occ_thre) == (occ_thre < 5e-3)
        ids, counts, pos = est._update(step, shell_occ_torch, occ_thre=occ_thre, ema_decay=0.95, warmup_steps=256,
                                       **dev_draws(d, step < 256))
        np.testing.assert_array_equal(host(counts), want["counts"])
        np.testing.assert_array_equal(host(ids), want["ids"])
        np.testing.assert_array_equal(bits(host(pos)), bits(want["positions"].reshape(-1, 3)))
        np.testing.assert_array_equal(bits(host(est.occs)), bits(want["occs"]))
        np.testing.assert_array_equal(host(est.binaries), want["binaries"])
        print(f"step {step}: thre {want['thre']:.6g}, nearest value {gap:.3g} away, {int(want['binaries'].sum())} occupied")


# ---- past the scans' first pass: res 65 (n_blk = 269: two blocks per scan thread; n_part = 269 at two levels) and the
# default res 128 (n_blk = 2048, n_part = 1024); tests/scan_refs.py, preconditions in tests/test_scan_refs_host.py -----------
@pytest.mark.parametrize("case", list(SR.CANDIDATE_CASES))
def test_candidates_equal_the_restatement_two_blocks_per_scan_thread(case):
    """test_candidates_equal_the_restatement's cases at res 65, the smallest resolution at which compact_scan_kernel gives
    each thread two blocks; the last compaction block is ragged (193 cells) and the scan threads from 135 on are idle."""
    from neurad_studio_amd import ops

    res = SR.OCC_RES_NEW
    c = SR.candidates_case(case, res)
    L, n, n_occ, warmup = c["L"], c["n"], c["n_occ"], c["warmup"]
    if case == "few_occupied":
        assert 0 < n_occ[0] <= n
    if case == "many_occupied":
        assert n_occ[0] > n
    if case == "two_levels":
        assert n_occ[0] > n >= n_occ[1] > 0
    grid = ops.OccGridSpec(torch.tensor(UNIT), cuda(c["binaries"]))
    ids, counts, pos = ops.occgrid_update_candidates(grid, cuda(c["occs"]), warmup, **dev_draws(c["draws"], warmup))
    assert ids.shape == (L, c["cap"]) and pos.shape == (L * c["cap"], 3)
    np.testing.assert_array_equal(host(counts), c["counts"])
    np.testing.assert_array_equal(host(ids), c["ids"])
    assert (c["ids"] == -1).any() and (c["occs"] < 0).any()


@pytest.mark.parametrize("box", [UNIT, [-1.3, -2.1, 0.2, 3.3, 1.7, 2.9]], ids=["power_of_two", "generic"])
def test_positions_lie_in_their_cells_at_res_65(box):
    """test_positions_lie_in_their_cells' rule at a resolution that is no power of two: within 4 ulp of the float64
    restatement and inside the cell's faces in the update's own fp32 arithmetic.  Bit-equality with the fp32 restatement is
    not required (1 / 65 is no fp32 number: whether the device's division rounds like numpy's is printed, not asserted)."""
    from neurad_studio_amd import ops

    res, L = SR.OCC_RES_NEW, 2
    occs, binaries = SR.grid_state(res, L, 21)
    d = UR.draws(res, L, False, 22)
    d["jitter"][0, :8] = np.float32(1.0 - 2.0 ** -24)  # the largest jitter there is
    d["jitter"][0, 8:16] = 0.0
    aabbs = UR.level_aabbs(box, L)
    grid = ops.OccGridSpec(torch.from_numpy(aabbs), cuda(binaries))
    ids, counts, pos = ops.occgrid_update_candidates(grid, cuda(occs), False, **dev_draws(d, False))
    ids, pos = host(ids), host(pos).reshape(L, -1, 3)
    want_ids, _ = UR.candidates(occs, binaries, res, L, False, None, d["cell_draws"], d["sel_draws"])
    np.testing.assert_array_equal(ids, want_ids)
    want32, want64 = UR.positions(aabbs, res, ids, d["jitter"]), UR.positions(aabbs, res, ids, d["jitter"], np.float64)
    flo, fhi = UR.cell_faces_f32(aabbs, res, ids)
    lo, hi = UR.cell_boxes(aabbs, res, ids)
    for l in range(L):
        ulp = float(np.spacing(np.float32(np.abs(aabbs[l]).max())))
        ok = ids[l] >= 0
        err = np.abs(pos[l].astype(np.float64) - want64[l])
        print(f"level {l}: max |p - float64 restatement| = {err[ok].max() / ulp:.2f} ulp; differs from the fp32 restatement on "
              f"{(bits(pos[l]) != bits(want32[l])).sum()} of {pos[l].size} coordinates")
        assert ok.sum() > 100000 and err.max() <= 4 * ulp
        assert np.all(pos[l][ok] >= flo[l][ok]) and np.all(pos[l][ok] <= fhi[l][ok])  # fp32 faces: exactly, any box
        assert np.all(np.abs(flo[l] - lo[l]) <= 4 * ulp) and np.all(np.abs(fhi[l] - hi[l]) <= 4 * ulp)
        centre = ((aabbs[l, :3] + aabbs[l, 3:]) * np.float32(0.5))
        np.testing.assert_array_equal(pos[l][~ok], np.broadcast_to(centre, pos[l][~ok].shape))


@pytest.mark.parametrize("regime", list(SR.EMA_OCC_THRE))
def test_ema_mean_and_threshold_over_more_than_256_partial_sums(regime):
    """res 65, two levels: 269 partial sums, so mean_final_kernel's threads go round their loop twice.  Injected candidates
    over the whole grid (tests/scan_refs.py: duplicates, untouched and invisible cells, a level with slots behind its count,
    values that are multiples of 2^-10, large only behind the first 256 partial sums).  occs bit for bit and the binaries
    on every cell against the restatement.  Precondition, from the restatement alone: no visible cell's value within 1e-3,
    relative, of the threshold."""
    from neurad_studio_amd import ops

    res, L, occ_thre = SR.OCC_RES_NEW, 2, SR.EMA_OCC_THRE[regime]
    assert SR.occ_sizes(res, L)[2] == 269
    c = SR.ema_case(res, L, seed=71)
    want = UR.ema(c["occs"], res, c["ids"], c["counts"], c["vals"], SR.EMA_DECAY)
    want_b, thre, mean = UR.threshold(want, occ_thre)
    gap = UR.threshold_gap(want, thre)
    print(f"mean {mean:.6g}, thre {thre:.6g}, nearest value {gap:.3g} away, {int(want_b.sum())} occupied")
    assert gap > 1e-3 and (mean > occ_thre) == (regime == "mean_above_occ_thre")
    stale = np.random.default_rng(72).random((L, res, res, res)) < 0.5  # every binary is rewritten, whatever it held
    grid = ops.OccGridSpec(torch.tensor(UNIT), cuda(stale))
    got = cuda(c["occs"])
    ops.occgrid_update_apply(grid, got, cuda(c["ids"]), cuda(c["counts"]), cuda(c["vals"]), SR.EMA_DECAY, occ_thre)
    np.testing.assert_array_equal(bits(host(got)), bits(want))
    np.testing.assert_array_equal(host(grid.binaries).reshape(-1), want_b)


@pytest.mark.parametrize("occ_thre", [1e-3, 1e-2])
def test_threshold_on_the_quantised_shell_at_the_default_resolution(occ_thre):
    """test_threshold_on_the_quantised_shell at OccGridEstimator's default resolution 128, one level: n_blk = 2048 (eight
    blocks per scan thread), n_part = 1024 (four rounds of the mean's loop).  In the unit box at a power-of-two resolution
    the position formula is exact up to one rounding, so the position bits are compared as well.  The restatement's mean
    lies above both thresholds here (tests/test_scan_refs_host.py), so thre = occ_thre at every step."""
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    est = OccGridEstimator(UNIT, resolution=128, levels=1)
    for step, d, want in SR.shell_run_default(occ_thre):
        gap = UR.threshold_gap(want["occs"], want["thre"])
        assert gap > 1e-3
        assert want["mean"] > occ_thre and want["thre"] == np.float32(occ_thre)
        ids, counts, pos = est._update(step, shell_occ_torch, occ_thre=occ_thre, ema_decay=0.95, warmup_steps=256,
                                       **dev_draws(d, step < 256))
        np.testing.assert_array_equal(host(counts), want["counts"])
        np.testing.assert_array_equal(host(ids), want["ids"])
        np.testing.assert_array_equal(bits(host(pos)), bits(want["positions"].reshape(-1, 3)))
        np.testing.assert_array_equal(bits(host(est.occs)), bits(want["occs"]))
        np.testing.assert_array_equal(host(est.binaries), want["binaries"])
        print(f"step {step}: thre {want['thre']:.6g}, nearest value {gap:.3g} away, {int(want['binaries'].sum())} occupied")


# ---- gating, state, hard conditions ----------------------------------------------------------------------------------------
def test_gating_first_update_and_state_dict_round_trip():
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    res, L = 16, 2
    est = OccGridEstimator(UNIT, resolution=res, levels=L)
    calls = []

    def half(p):
        calls.append(p.shape)
        return torch.full((p.shape[0], 1), 0.5, device=p.device)

    est.update_every_n_steps(step=7, occ_eval_fn=half, n=16)
    assert not calls and bool(est.fresh) and bool((est.occs == 1).all())
    est.eval()
    with pytest.raises(RuntimeError):
        est.update_every_n_steps(step=0, occ_eval_fn=half)
    est.train()
    est.update_every_n_steps(step=0, occ_eval_fn=half, n=16)
    assert calls == [(L * res ** 3, 3)] and not bool(est.fresh)
    # the EMA started from zero: max(0 * 0.95, 0.5), not max(1 * 0.95, 0.5)
    assert bool((est.occs == 0.5).all()) and bool(est.binaries.all())
    est.update_every_n_steps(step=32, occ_eval_fn=shell_occ_torch, warmup_steps=16, n=16)
    # after warm-up only the candidates are touched: decayed once (the shell's values are far below), the rest keeps 0.5
    assert set(np.unique(host(est.occs)).tolist()) == {float(np.float32(0.5) * np.float32(0.95)), 0.5}
    # round trip: a new estimator with the saved state makes the same next update, bit for bit
    sd = {k: v.clone() for k, v in est.state_dict().items()}
    other = OccGridEstimator([-3, -3, -3, 3, 3, 3], resolution=res, levels=L)
    other.load_state_dict(sd)
    assert not bool(other.fresh) and torch.equal(other.aabbs, est.aabbs)
    d = UR.draws(res, L, False, 41)
    for e in (est, other):
        e._update(48, shell_occ_torch, occ_thre=0.49, warmup_steps=16, **dev_draws(d, False))  # thre = the mean
    assert torch.equal(est.occs.view(torch.int32), other.occs.view(torch.int32)) and torch.equal(est.binaries, other.binaries)
    assert 0 < int(est.binaries.sum()) < L * res ** 3
    assert not torch.equal(est.occs, sd["occs"])
    # in-place edits of the binaries are what the march sees
    est.binaries[:] = False
    o = torch.zeros(8, 3, device="cuda")
    dirs = torch.nn.functional.normalize(cuda(synth.normal((8, 3), 5)), dim=-1)
    assert est.sampling(o, dirs, render_step_size=0.1)[0].numel() == 0


def test_update_is_reproducible_and_does_not_synchronise():
    """Same state, same draws -> the same bits; from the second call on no host synchronisation (which also rules out an
    allocation sized by data: its size would have to be read back)."""
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    res, L = 16, 2
    runs = []
    for _ in range(2):
        est = OccGridEstimator(UNIT, resolution=res, levels=L)
        for i, step in enumerate([0, 16, 32, 48]):
            d = UR.draws(res, L, step < 32, 50 + i)
            est._update(step, shell_occ_torch, warmup_steps=32, **dev_draws(d, step < 32))
        runs.append((est.occs.clone(), est.binaries.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])
    trivial = lambda p: p[:, :1].abs() * 0.01  # noqa: E731
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in (16, 64, 80):  # warm-up and later, draws made on the device
            est._update(step, trivial, warmup_steps=32)
        est.train()
        est.update_every_n_steps(96, trivial, warmup_steps=32)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(est.occs).all()


# ---- multi-level march -----------------------------------------------------------------------------------------------------
def march_inputs(R, seed, spread):
    o = (synth.normal((R, 3), seed) * np.asarray(spread)).astype(np.float32)
    d = synth.normal((R, 3), seed + 1)
    d[:5, 0] = 0.0
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return o, d


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_one_level_is_the_single_grid_march(cone):
    from neurad_studio_amd import ops

    res, R = 32, 200
    binaries = np.random.default_rng(0).random((res, res, res)) < 0.3
    aabb = torch.tensor([-10.0, -10, -2, 10, 10, 6])
    o, d = march_inputs(R, 1, [6.0, 6.0, 2.0])
    t_max = cuda(synth.uniform((R,), 5.0, 60.0, 3))
    args = (cuda(o), cuda(d), 0.25)
    kw = dict(near_plane=0.1, far_plane=40.0, t_max=t_max, cone_angle=cone)
    single = ops.occgrid_march(ops.OccGridSpec(aabb, cuda(binaries)), *args, **kw)
    levels = ops.occgrid_march(ops.OccGridSpec(aabb[None], cuda(binaries[None])), *args, **kw)
    assert single[0].numel() > 1000
    for a, b in zip(single, levels):
        assert torch.equal(a, b) if a.dtype == torch.int64 else torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_three_level_march_vs_restatement(cone):
    """Every candidate interval whose float64 midpoint is further than 1e-4 (in cells) from a cell face and from every level's
    box is kept or dropped exactly as the restatement says; at most 0.5 % may be that close (expected: about 6e-4)."""
    from neurad_studio_amd import ops

    res, L, R, step = 16, 3, 160, 0.11
    rng = np.random.default_rng(7)
    binaries = rng.random((L, res, res, res)) < np.reshape([0.35, 0.5, 0.65], (L, 1, 1, 1))
    aabbs = UR.level_aabbs(UNIT, L)
    o, d = march_inputs(R, 8, [0.9, 0.9, 0.9])
    o[:20] *= 4.0  # some origins in the outer levels and outside the grid
    ri, ts, te, seg = ops.occgrid_march(ops.OccGridSpec(torch.from_numpy(aabbs), cuda(binaries)), cuda(o), cuda(d), step,
                                        near_plane=0.05, far_plane=30.0, cone_angle=cone)
    ri, ts, te = host(ri), host(ts), host(te)
    m = UR.march_levels(aabbs, binaries, o, d, step, 0.05, 30.0, cone_angle=cone)
    share = m["ambiguous"].mean()
    print(f"{len(m['ray'])} candidates, {m['keep'].sum()} kept, {len(ri)} emitted, ambiguous share {share:.2e}")
    assert len(m["ray"]) > 4000 and share <= 0.005
    emitted = np.zeros(len(m["ray"]), bool)
    first = np.searchsorted(m["ray"], np.arange(R + 1))
    tol = 4 * 2.0 ** -23 * 30.0  # candidates are a step apart; powf may differ from the restatement's by an ulp or two
    for r in range(R):
        cand_ts = m["t_start"][first[r]:first[r + 1]]
        mine = ri == r
        if not mine.any():
            continue
        assert len(cand_ts), f"ray {r}: samples from a ray the restatement never marches"
        k = np.abs(ts[mine][:, None] - cand_ts[None]).argmin(1)
        assert np.all(np.diff(k) > 0)
        assert np.abs(ts[mine] - cand_ts[k]).max() <= tol and np.abs(te[mine] - m["t_end"][first[r]:first[r + 1]][k]).max() <= tol
        if cone == 0.0:
            np.testing.assert_array_equal(bits(ts[mine]), bits(cand_ts[k]))
        emitted[first[r] + k] = True
    sure = ~m["ambiguous"]
    np.testing.assert_array_equal(emitted[sure], m["keep"][sure])
    assert np.all(np.diff(ri) >= 0) and int(seg[-1]) == len(ri)


# ---- invisible cells -------------------------------------------------------------------------------------------------------
def test_mark_invisible_cells_vs_restatement():
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    K, c2w, w, h = UR.cameras()
    res, L, near = 32, 2, 0.5
    assert len(c2w) >= 8 and (np.abs(c2w[:, :, 3]).max(1) < 4).any()  # some cameras inside the grid
    est = OccGridEstimator([-4, -4, -4, 4, 4, 4], resolution=res, levels=L)
    c2w44 = np.concatenate([c2w, np.tile(np.array([[[0, 0, 0, 1]]], np.float32), (len(c2w), 1, 1))], 1)
    est.mark_invisible_cells(torch.from_numpy(K), torch.from_numpy(c2w44), w, h, near_plane=near)
    aabbs = host(est.aabbs)
    v64, amb = UR.mark_invisible(aabbs, res, K, c2w, w, h, near, dtype=np.float64, margin=1e-3)
    got = host(est.occs)
    assert not bool(est.fresh) and set(np.unique(got)) == {-1.0, 0.0}
    print(f"visible {v64.mean():.3f}; left out {amb.mean():.5f}; differs from the fp32 restatement on "
          f"{((got == 0) != UR.mark_invisible(aabbs, res, K, c2w, w, h, near)).sum()} cells")
    assert amb.mean() <= 0.01
    np.testing.assert_array_equal((got == 0)[~amb], v64[~amb])
    b = host(est.binaries).reshape(-1)
    np.testing.assert_array_equal(b, got == 0)  # an invisible cell is never occupied; the visible ones stay "unknown"
    # one K for all cameras, [N,3,4] poses
    est2 = OccGridEstimator([-4, -4, -4, 4, 4, 4], resolution=res, levels=L)
    est2.mark_invisible_cells(torch.from_numpy(K[:1]), torch.from_numpy(c2w), w, h, near_plane=near)
    v1, amb1 = UR.mark_invisible(aabbs, res, K[:1], c2w, w, h, near, dtype=np.float64, margin=1e-3)
    np.testing.assert_array_equal((host(est2.occs) == 0)[~amb1], v1[~amb1])
    # invisible cells are never evaluated and never written by an update
    seen = []
    est.train()
    est.update_every_n_steps(0, lambda p: seen.append(p) or torch.ones_like(p[:, :1]))
    after = host(est.occs)
    np.testing.assert_array_equal(after[got < 0], -1.0)
    np.testing.assert_array_equal(after[got == 0], 1.0)
    assert not host(est.binaries).reshape(-1)[got < 0].any()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_pruned_route_end_to_end():
    """Density = an indicator over whole level-0 cells.  One warm-up update finds exactly that set, the march then emits
    exactly the restatement's samples -- fewer than before -- and the packed render of the pruned samples agrees with the
    unpruned one (the dropped samples weigh exactly zero; only the scan's association differs)."""
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples
    from neurad_studio_amd.model_components.renderers import render_packed
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    res, R, step = 16, 96, 0.07
    rng = np.random.default_rng(3)
    inside = rng.random((res, res, res)) < 0.25
    inside_t = cuda(inside)

    def cell_of(p):
        i = torch.clamp(torch.floor((p + 1.0) / 2.0 * res).long(), 0, res - 1)
        return inside_t[i[:, 0], i[:, 1], i[:, 2]]

    sigma = lambda p: cell_of(p).float()[:, None] * 6.0  # noqa: E731
    o, d = march_inputs(R, 60, [0.5, 0.5, 0.5])
    o_t, d_t = cuda(o), cuda(d)
    est = OccGridEstimator(UNIT, resolution=res)
    before = est.sampling(o_t, d_t, render_step_size=step)
    jitter = np.random.default_rng(4).random((1, res ** 3, 3), dtype=np.float32) * np.float32(0.999)  # strictly inside
    est._update(0, lambda p: sigma(p) * step, jitter=cuda(jitter))
    np.testing.assert_array_equal(host(est.binaries[0]), inside)
    after = est.sampling(o_t, d_t, render_step_size=step, stratified=False)
    m = UR.march_levels(np.asarray([UNIT], np.float32), inside[None], o, d, step)
    k = m["keep"]
    np.testing.assert_array_equal(host(after[0]), m["ray"][k])
    np.testing.assert_array_equal(bits(host(after[1])), bits(m["t_start"][k]))
    np.testing.assert_array_equal(bits(host(after[2])), bits(m["t_end"][k]))
    assert 0 < after[0].numel() < before[0].numel()

    def render(ri, ts, te):
        p = o_t[ri] + d_t[ri] * ((ts + te) * 0.5)[:, None]
        feat = torch.cat([torch.sin(3.0 * p), torch.cos(2.0 * p), p], -1).contiguous()
        rs = RaySamples(frustums=Frustums(origins=o_t[ri], directions=d_t[ri], starts=ts[:, None], ends=te[:, None],
                                          pixel_area=torch.ones_like(ts[:, None])))
        return render_packed(feat, rs, ri, R, density=sigma(p))

    full, pruned = render(*before), render(*after)
    for key in ("features", "depth", "accumulation"):
        err = rel_l2(host(pruned[key]), host(full[key]))
        print(f"{key}: pruned vs unpruned {err:.3g}")
        assert err < TIGHT, key
    assert float(full["accumulation"].max()) > 0.5


# ---- density_fn ------------------------------------------------------------------------------------------------------------
def test_density_fn_equals_get_density_and_feeds_the_update():
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples
    from neurad_studio_amd.fields.neurad_field import NeuRADProposalField, NeuRADProposalFieldConfig
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    lg = 11
    c = NeuRADProposalFieldConfig()
    c.grid.static.log2_hashmap_size = lg
    fld = NeuRADProposalField(c, actors=None, static_scale=10.0).cuda()
    w, _ = synth.linear(1, 6, 72, bias=False)
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.copy_(cuda(synth.hash_table(6 * 2 ** lg, 1, seed=71, scale=2.0)))
        fld.density_decoder.weight.copy_(cuda(w + np.float32(0.3)))
    p = cuda(synth.normal((500, 3), 73) * 8.0)
    zero = torch.zeros_like(p[:, None, :1])
    rs = RaySamples(frustums=Frustums(origins=p[:, None], directions=torch.ones_like(p[:, None]), starts=zero, ends=zero,
                                      pixel_area=torch.ones_like(zero)))
    with torch.no_grad():
        want = fld.get_density(rs)[0]
        got = fld.density_fn(p)
        got2 = fld.density_fn(p.reshape(50, 10, 3))
    assert got.shape == (500, 1) and got2.shape == (50, 10, 1)
    assert torch.equal(got, want.reshape(500, 1)) and torch.equal(got2.reshape(500, 1), got)
    assert float(got.std()) > 0 and torch.isfinite(got).all()
    est = OccGridEstimator([-8, -8, -8, 8, 8, 8], resolution=16, levels=2)
    fld.train()
    jitter = cuda(np.random.default_rng(5).random((2, 16 ** 3, 3), dtype=np.float32))
    est.update_every_n_steps(0, occ_eval_fn=fld.density_fn)
    prev = est.occs.clone()
    ids, counts, pos = est._update(16, fld.density_fn, occ_thre=1e9, jitter=jitter)  # thre = the mean of the densities
    with torch.no_grad():
        dens = fld.density_fn(pos).reshape(-1)
    assert not bool(est.fresh) and fld.hashgrid.static_grid.hash_table.grad is None
    # a warm-up update of a grid without invisible cells: cell c's one candidate sits in slot c
    assert torch.equal(ids.long(), torch.arange(16 ** 3, device="cuda").expand(2, -1)) and counts.tolist() == [16 ** 3] * 2
    assert torch.equal(est.occs, torch.maximum(prev * 0.95, dens))
    assert 0 < int(est.binaries.sum()) < 2 * 16 ** 3
