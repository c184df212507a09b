"""The helpers of the exact hash-grid family (hashgrid_exact_refs.py), checked on the CPU: every case satisfies the premises
that make its answer unique (``assert_exact_*``), every census is non-zero where a device test relies on it, the restated
hash equals the oracle's, and the reference is SENSITIVE -- each mutant (a defect a kernel could have) changes at least one
element of every forward case and one entry of every scatter case."""
import itertools

import numpy as np
import pytest

import hashgrid_exact_refs as H
import neurad_oracle as O

FS = (1, 2, 4, 8)
SIZES = (1, 85, 86)  # n L = 3, 255, 258 around the 256-thread workgroup (and 128: a wave boundary inside a sample)
MUTANTS = ([("swap", a, b) for a, b in itertools.combinations(range(8), 2)] + [("floor_for_ceil", a) for a in range(3)] +
           [("flip_o", a) for a in range(3)] + [("drop_last",), ("drop_term",), ("dup_sample",), ("level",)])


def _cases():
    for name in H.FWD_GRIDS:
        for F in FS:
            for n in SIZES:
                yield H.scatter_case(name, F, n)


def _ids(c):
    return c.name


def test_the_table_formula_separates_the_rows_of_every_block():
    g = H.Grid(3, 16, 64, 8, 1)
    t = H.table_values(g)[:, 0].reshape(-1, 4)
    assert t.min() >= -64 and t.max() < 64
    assert all(len(set(r)) == 4 for r in t.tolist())
    assert (H.table_at(g, np.arange(g.rows))[:, 0] == H.table_values(g)[:, 0]).all()
    assert (H.table_values(g).astype(np.float16).astype(np.int64) == H.table_values(g)).all()


@pytest.mark.parametrize("name", list(H.FWD_GRIDS))
def test_the_restated_hash_is_the_oracles(name):
    c = H.forward_case(name, 1, 257)
    idx, o = H.own_indices(c.x, c.grid.scal, c.grid.T)
    ref, o32 = O.hashgrid_corner_indices(c.x, c.grid.scal, c.grid.T)
    assert (idx == ref).all() and (o == o32).all()


@pytest.mark.parametrize("case", list(_cases()), ids=_ids)
def test_every_case_is_exact(case):
    qf = H.assert_exact_forward(case.grid, case.x)
    qs = H.assert_exact_scatter(case.grid, case.x, case.go, partition=True)
    assert 2.0 ** -24 <= min(qf, qs) <= 1.0
    # the fp32 oracle forward is the float64 lerp, bit for bit; the float64 scatter-add is an fp32 number
    table = H.table_values(case.grid).astype(np.float32)
    assert (O.hashgrid_fwd(case.x, table, case.grid.scal, case.grid.T).astype(np.float64) == H.forward_ref(case.grid, case.x)).all()
    s = H.scatter_ref(case.grid, case.x, case.go)
    assert (s == s.astype(np.float32)).all()


@pytest.mark.parametrize("case", [c for c in _cases() if c.n > 1], ids=_ids)
def test_the_reference_sees_every_mutant(case):
    fwd, sc = H.forward_ref(case.grid, case.x), H.scatter_ref(case.grid, case.x, case.go)
    for m in MUTANTS:
        f2 = H.forward_ref(case.grid, case.x, m)
        assert not np.array_equal(fwd, f2, equal_nan=True), ("forward", m)
        assert not np.array_equal(sc, H.scatter_ref(case.grid, case.x, case.go, m)), ("scatter", m)


@pytest.mark.parametrize("F", FS)
def test_the_single_sample_cases_see_the_sample_mutants(F):
    """one sample cannot separate all 28 slot swaps on every grid (its 8 corners need 8 different values and weights); it is
    there for the launch's lower edge, and sees every mutant that removes, doubles or rescales the sample"""
    for name in H.FWD_GRIDS:
        case = H.scatter_case(name, F, 1)
        fwd, sc = H.forward_ref(case.grid, case.x), H.scatter_ref(case.grid, case.x, case.go)
        for m in [("drop_last",), ("drop_term",), ("dup_sample",), ("level",)] + [("flip_o", a) for a in range(3)]:
            assert not np.array_equal(fwd, H.forward_ref(case.grid, case.x, m), equal_nan=True), (name, m)
            assert not np.array_equal(sc, H.scatter_ref(case.grid, case.x, case.go, m)), (name, m)


@pytest.mark.parametrize("half", (False, True))
@pytest.mark.parametrize("name", ("wave", "block2"))
def test_paired_load_census(name, half):
    c = H.forward_case(name, 1, 86)
    s = H.census_paired(c.grid, c.x, half)
    assert all(v > 0 for v in s["classes"].values()) and s["other"] > 0 and s["full_waves"] > 0
    assert s["combos"] == H.admitted_combos(c.grid, half)
    assert 0.6 < s["same"] / (s["same"] + s["other"]) < 0.9 or half


def test_one_block_tables_take_only_the_same_branch():
    c = H.forward_case("block1", 1, 86)
    s = H.census_paired(c.grid, c.x, False)
    assert s["other"] == 0 and s["combos"] == H.admitted_combos(c.grid, False) and all(v > 0 for v in s["classes"].values())


def test_position_census():
    s = H.census_positions(*_gx(H.forward_case("wave", 1, 86)))
    assert all(v > 0 for v in s["lattice"].values()) and s["below"] and s["above"] and s["zero"] and s["one"]
    s = H.census_positions(*_gx(H.forward_case("fine", 1, 128)))
    assert s["high_bits"] > 0 and s["distinct8"] > 0 and sum(s["lattice"].values()) == 0


def _gx(c):
    return c.grid, c.x


@pytest.mark.parametrize("R,S", [(1, 1), (9, 7), (1, 64), (2, 64), (13, 5), (257, 1)])
def test_dense_ray_positions_are_exact_and_scatter_exactly(R, S):
    r = H.dense_rays(R, S, 8, seed=R)
    x = H.ray_positions(r)
    g = H.Grid(3, 16, 64, 8, 2)
    H.assert_exact_scatter(g, x, H.small_grads(len(x), g.width, 0), partition=True)
    if R >= 9:  # the still rays: |u|_inf exactly 2 and 4 land on 7/8, 1/8, 15/16, 1/16
        assert {0.875, 0.125, 0.9375, 0.0625} <= set(np.unique(x).tolist())


@pytest.mark.parametrize("S", (16, 64, 256))
def test_fan_rays_are_coherent_and_exact(S):
    r = H.dense_rays(H.CHUNK // S, S, 8, 0, mode="fan")
    x = H.ray_positions(r)
    assert H.coherent_chunk(r, 0, H.CHUNK) == H.CHUNK // S and H.coherent_chunk(r, 0, H.CHUNK - 1) == 0
    for F in FS:
        g = H.Grid(3, 16, 64, 8, F)
        H.assert_exact_scatter(g, x, H.small_grads(len(x), g.width, 0, gmax=2), partition=True)


def test_packed_rays_follow_the_marchs_convention():
    r = H.packed_rays((0, 3, 0, 0, 17, 1, 0, 64, 5, 0), 8, 0)
    assert (np.diff(r.ray_of) >= 0).all() and set(r.ray_of.tolist()) == {1, 4, 5, 7, 8} and len(r.starts) == 90
    H.ray_positions(r)


def test_run_censuses():
    c = H.run_rows_case(2, 257)
    off = H.row_offsets(c)
    s = H.census_runs(c.grid, c.x, 16, key_extra=c.grid_id, live=off >= 0)
    assert s["merged"] > 0 and s["across"] > 0 and s["other_grid"] > 0 and s["longest"] >= 4
    assert (off[[38, 40, 50, 51]] < 0).all() and (off[[36, 37, 39, 41, 48, 49]] >= 0).all()
    H.assert_exact_scatter(c.grid, c.x, c.go, partition=True, row_offset=off, rows=3 * c.grid.rows)
    r = H.dense_rays(2, 64, 8, 3)
    r.origins[:], r.directions[:] = r.origins[1], 0.0  # two still rays at one point: a run of 64, and equal keys at 63 | 64
    s = H.census_runs(H.Grid(3, 16, 64, 8, 1), H.ray_positions(r), 64)
    assert s["longest"] == 64 and s["across"] == 3 * 8
    s = H.census_runs(H.Grid(3, 16, 64, 8, 1), H.ray_positions(H.dense_rays(257, 1, 8, 257)), 64)
    assert s["groups_without_run"] > 0


def test_the_plan_restatement_matches_the_library():
    """bin_plan against the workspace query (host logic of the library): the record area is n * rec_slots * L * record bytes"""
    import ctypes

    import __graft_entry__ as ge

    lib = ctypes.CDLL(ge.LIB)
    from neurad_studio_amd import _lib

    for (L, lo, hi, lg, F), n in itertools.product([(3, 16, 64, 8, 1), (6, 16, 512, 12, 1), (1, 16, 16, 10, 4), (3, 16, 1024, 12, 1),
                                                    (2, 5, 11, 2, 8)], (1, 4097, 64 * 4096 + 1)):
        g = H.Grid(L, lo, hi, lg, F)
        p = H.bin_plan(g, n)
        c = _lib.Grid()
        c.num_levels, c.n_features, c.log2_table_size, c.param_dtype = L, F, lg, 0
        for i, v in enumerate(g.scal.tolist()):
            c.scalings[i] = v
        need = ctypes.c_int64(0)
        assert lib.nrhip_encode_bwd_binned_workspace(ctypes.byref(c), ctypes.c_int64(n), ctypes.byref(need)) == 0
        rec = n * p["rec_slots"] * L * ((2 if p["pair"] else 1) * F + 1) * 4
        cols = L * p["nb"]
        book = sum(-(-b // 256) * 256 for b in (p["chunks"] * cols * 4, p["nseg"] * cols * 4, cols * 4, (cols + 1) * 4,
                                                 L * p["chunks"] * 16 * 4, p["chunks"] * 4096 * 16, p["chunks"] * 4096 * 2, p["chunks"] * 4))
        assert need.value == rec + book, (g, n, p)
    assert H.bin_plan(H.Grid(6, 16, 512, 12, 1), 4097)["lgroups"] == 6  # 512 wanted, bumped to a divisor of L
    assert H.bin_plan(H.Grid(3, 16, 1024, 12, 1), 4097)["rec_slots"] == 8  # a resolution that reaches the slice length
