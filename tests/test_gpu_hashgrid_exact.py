"""Bit-for-bit tests of the standalone hash-grid kernels against the int64 / float64 reference of hashgrid_exact_refs.py
(which explains why every element has ONE right answer on the dyadic lattice, whatever the order of the sums).

Every output buffer is prefilled with NaN (accumulating entry points: with what the case says), has a guard row behind it
that must stay NaN, and every call runs twice with the second run held to the first.  Zeros must be +0.0: comparisons are on
the bit patterns.

branch -> shape, and the census / query that shows the branch is reached
---------------------------------------------------------------------------------------------------------------------------
forward, thread per (sample, level), 256 threads
  last workgroup partly filled / exactly full   wave n = 85, 86 (n L = 255, 258), mixed n = 128 and four n = 64 (256), one n = 257
                                                (n L = 256 and 257 are no multiples of L = 3); n = 1
  F x storage dispatch                          every F in {1, 2, 4, 8} x {fp32, fp16} at every shape
  positions 0, 1, lattice on 1 / 2 / 3 axes,    census_positions: lattice[1], [2], [3], zero, one, below, above > 0
    [-1, 0) and (1, 2]
  load_corners_f1 `same` | second load          census_paired: every class, `other` and >= 1 wave holding all of them
    every (rf & 3, rc & 3) under `same`         census_paired()["combos"] == admitted_combos()
    one block per level (log2 T = 2)            block1 / odd: other == 0
  hashed fine levels                            fine: census_positions high_bits > 0, distinct8 > 0, no lattice point
  byte offsets in [2^31, 2^32)                  the 4 GiB grid (L = 16, log2 T = 24, F = 4): census offset_2g > 0
  hashgrid_multi_fwd                            3 grids, ids interleaved and sorted
  encode_fwd                                    dense rays incl. |u|_inf = 1, 2, 4 with ties (ray_positions asserts exactness)
position gradient (hashgrid_bwd_input, _multi)  F x storage at n = 255, 256, 257 on the coarse lattice (input_grad_ref bound)
atomic scatter
  hashgrid_bwd                                  the forward shapes
  encode_bwd, 64-lane runs                      (13, 5): several rays a wave; (2, 64) still rays: census_runs longest == 64,
                                                across == 24 (63 | 64 must not merge); (257, 1): groups_without_run > 0;
                                                n = 1, 63, 64, 65, 257: dead lanes clamp to sample n - 1
  hashgrid_multi_bwd, DPP rows / plain          run_rows_case: census_runs(16) merged, across (15 | 16), other_grid > 0; ids -1
                                                and n_grids and the absent grid 2 inside runs (row_offsets < 0 there)
the partition (pairs = all | none at every F)
  chunks 1, 2                                   n = 1, 4095, 4096, 4097
  nlive = 1024 | 1025 | 0                       live_per_chunk == [1024, 0, 1025, 1]
  one level a workgroup | several; segments     bin_plan: L = 6 n = 4097 lgroups == 6; n = 341 * 4096 + 1: lgroups == 3, nseg == 6;
                                                n = 255 * 4096 + 1: 4 groups wanted, bumped to 6
  more than 64 chunks, L = 1                    n = 64 * 4096 + 1: bin_plan nseg == 2
  rec_slots == 8, pairs across two slices       sliced grid: bin_plan rec_slots == 8, census_slices straddle > 0
  cnt == 0 fill, float4 | scalar | fp16         census_slices empty > 0; all-silent batches on log2 T = 1 (F = 1: 2 floats a slice)
  rounds                                        NRHIP_BIN_ROUND_LOG2 = 15, n = 2^15 + 1 and 2^16: bin_plan rounds == 2
  overwrite 1 | 0                               NaN prefill | prefill 3 -> 3 + reference
  rows_are_zero                                 widths 8, 32 (aligned and one float off), 64; +0.0 and -0.0 rows
  walk order                                    fan rays S = 16, 64, 256: coherent_chunk == 4096 / S; NRHIP_BIN_TRANSPOSE 1 | 0
  packed source                                 ragged segments with empty rays
  multi-grid                                    slot_of < 0, ids out of range, n_slots < n_grids; block [slot][L T][F]
  fp16 output                                   integers, +-inf beyond 65504, the refusal of a second round (overwrite = 0 with an
                                                fp16 gradient cannot be asked for through the C ABI: the _f16 forms take no flag)
"""
from dataclasses import replace

import numpy as np
import pytest
import torch

import hashgrid_exact_refs as H
from neurad_studio_amd import _lib, ops

pytestmark = pytest.mark.gpu

FS = (1, 2, 4, 8)
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spec_of(g: H.Grid) -> ops.GridSpec:
    return ops.GridSpec(g.L, g.F, g.lg, g.min_res, g.max_res)


def table_of(g: H.Grid, half: bool, copies: int = 1):
    """the formula table(s) on the device: [copies][rows, F]; copy c holds the rows c * rows ... of the formula table"""
    return [torch.from_numpy(H.table_values(replace(g, row0=c * g.rows))).to(torch.float16 if half else torch.float32).cuda()
            for c in range(copies)]


def guarded(rows: int, width: int, fill=NAN, dtype=torch.float32):
    """-> (the whole buffer with one guard row of NaN behind ``rows`` rows of ``fill``, the view the kernel writes)"""
    buf = torch.full((rows + 1, width), NAN, device="cuda", dtype=dtype)
    buf[:rows] = fill
    return buf, buf[:rows]


def bits(a: np.ndarray):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def held(buf, ref64: np.ndarray, what: str):
    """the buffer's rows equal the float64 reference bit for bit (the reference must be a number of the buffer's type, or
    beyond its largest: inf), the guard row is still NaN"""
    got = buf.cpu().numpy()
    body, guard = got[:-1], got[-1]
    assert np.isnan(guard.astype(np.float64)).all(), f"{what}: the guard row was written"
    with np.errstate(over="ignore"):
        exp = ref64.reshape(body.shape).astype(body.dtype)
    ok = (exp.astype(np.float64) == ref64.reshape(body.shape)) | np.isinf(exp.astype(np.float64))
    assert ok.all(), f"{what}: the reference is not exact in the output type"
    bad = np.argwhere(bits(body) != bits(exp))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {body.size} elements differ, first at {bad[:5].tolist()}: got "
                           f"{[float(body[tuple(b)]) for b in bad[:5]]}, expected {[float(exp[tuple(b)]) for b in bad[:5]]}")
    return got


def twice(run, what: str):
    a = run()
    b = run()
    torch.cuda.synchronize()
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), f"{what}: the second run differs from the first"
    return a


def dense(r: H.Rays):
    t = [dev(a) for a in (r.origins, r.directions, r.area, r.starts, r.ends)]
    return ops._c_rays(*t)


def packed(r: H.Rays):
    t = [dev(a) for a in (r.origins, r.directions, r.area, r.starts, r.ends)]
    c, keep = ops._c_packed_rays("test", *t)
    return c, (keep, dev(r.ray_of))


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
FWD_SHAPES = [("wave", 1), ("wave", 85), ("wave", 86), ("mixed", 128), ("one", 257), ("block1", 86), ("block2", 86), ("odd", 86),
              ("fine", 128), ("four", 64), ("wave9", 86)]


@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("name,n", FWD_SHAPES)
def test_forward(name, n, F, half):
    case = H.forward_case(name, F, n)
    g = case.grid
    H.assert_exact_forward(g, case.x)
    cp = H.census_positions(g, case.x)
    if name == "fine":
        assert cp["high_bits"] > 0 and cp["distinct8"] > 0 and sum(cp["lattice"].values()) == 0
    elif n >= 85:
        assert all(v > 0 for v in cp["lattice"].values()) and cp["zero"] and cp["one"] and cp["below"] and cp["above"]
    if F == 1 and n >= 85:
        s = H.census_paired(g, case.x, half)
        if name in ("wave", "block2"):
            assert all(v > 0 for v in s["classes"].values()) and s["other"] > 0 and s["full_waves"] > 0
            assert s["combos"] == H.admitted_combos(g, half)
        if name in ("block1", "odd") and not half:
            assert s["other"] == 0 and s["combos"] == H.admitted_combos(g, half)
    spec, x = spec_of(g), dev(case.x)
    (table,) = table_of(g, half)
    ref = H.forward_ref(g, case.x)

    def run():
        buf, out = guarded(n, g.width)
        ops.launch("nrhip_hashgrid_fwd", spec.c_grid(table), table, x, n, out)
        return buf

    held(twice(run, case.name), ref, case.name)

    # three grids, ids interleaved and sorted: sample i looks into tables[id[i]]
    tables = table_of(g, half, 3)
    for order in (False, True):
        gid = H.multi_ids(n, 3, 1, order, strays=False)
        mref = np.zeros((n, g.width))
        for c in range(3):
            mref[gid == c] = H.forward_ref(replace(g, row0=c * g.rows), case.x[gid == c])
        ids = dev(gid)

        def run_multi():
            buf, out = guarded(n, g.width)
            ops.launch("nrhip_hashgrid_multi_fwd", spec.c_grid(tables[0]), ops._ptr_array(tables), 3, ids, x, n, out)
            return buf

        held(twice(run_multi, case.name + " multi"), mref, case.name + " multi")


@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R,S", [(1, 1), (17, 5), (43, 2), (2, 64)])
def test_encode_forward(R, S, F, half):
    g = H.Grid(3, 16, 64, 8, F)
    r = H.dense_rays(R, S, 8, seed=R)
    pos = H.ray_positions(r)
    H.assert_exact_forward(g, pos)
    if R >= 17:
        assert {0.875, 0.125, 0.9375, 0.0625} <= set(np.unique(pos).tolist())  # |u|_inf = 2 and 4 are there
    spec = spec_of(g)
    (table,) = table_of(g, half)
    rays, keep = dense(r)

    def run():
        buf, out = guarded(R * S, g.width)
        ops.launch("nrhip_encode_fwd", spec.c_grid(table), table, H.STATIC_SCALE, rays, out)
        return buf

    held(twice(run, "encode_fwd"), H.forward_ref(g, pos), "encode_fwd")


def test_the_largest_fp32_grid():
    """L = 16, log2 T = 24, F = 4: 4 GiB, byte offsets row * 16 up to 2^32 - 16.  hashgrid_fwd on the 2^-5 lattice, and
    hashgrid_bwd_input on the 2^-1 lattice with one live level per sample (scal * d adds 13 bits)."""
    g = H.Grid(16, 16, 8192, 24, 4)
    n = 257
    table = torch.empty((g.rows, g.F), device="cuda", dtype=torch.float32)
    step = 1 << 22
    f = torch.arange(g.F, device="cuda", dtype=torch.int64)[None, :]
    for a in range(0, g.rows, step):
        table[a:a + step] = H.table_formula(torch.arange(a, a + step, device="cuda", dtype=torch.int64)[:, None], f, g.F).float()
    spec = spec_of(g)
    x = H.lattice_positions(n, 5, 11)
    H.assert_exact_forward(g, x)
    cp = H.census_positions(g, x)
    assert cp["offset_2g"] > 1000 and cp["high_bits"] > 0
    xd = dev(x)

    def run():
        buf, out = guarded(n, g.width)
        ops.launch("nrhip_hashgrid_fwd", spec.c_grid(table), table, xd, n, out)
        return buf

    held(twice(run, "4 GiB forward"), H.forward_ref(g, x), "4 GiB forward")

    x1 = H.lattice_positions(n, 1, 12, edges=False)
    x1[::5] = (x1[::5] + np.float32(0.5)) % np.float32(1.5)  # 0, 1/2 and 1 on every axis
    go = np.zeros((n, g.L, g.F), np.float32)
    i = np.arange(n)
    go[i, i % g.L, i % g.F] = np.where(i % 2, 1.0, -1.0)
    go = go.reshape(n, -1)
    ref, mag, q = H.input_grad_ref(g, x1, go)
    assert mag.max() < H.LIMIT * q and np.abs(ref).max() > 0
    x1d, god = dev(x1), dev(go)

    def run_dx():
        buf, out = guarded(n, 3)
        ops.launch("nrhip_hashgrid_bwd_input", spec.c_grid(table), table, x1d, god, n, out)
        return buf

    held(twice(run_dx, "4 GiB bwd_input"), ref, "4 GiB bwd_input")
    del table
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# position gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", (255, 256, 257))
def test_position_gradient(n, F, half):
    """every elementary term scal * go * value * o_a * o_b is a multiple of the quantum and every sum of their absolute values
    is below 2^24 quanta (input_grad_ref), so every partial sum of the kernel's tree is exact: K = 3 on (12, 40), go in +-1"""
    g = H.Grid(2, 12, 40, 6, F)
    x = H.lattice_positions(n, 3, n)
    go = H.small_grads(n, g.width, n, gmax=1)
    ref, mag, q = H.input_grad_ref(g, x, go)
    assert mag.max() < H.LIMIT * q and (ref != 0).sum() > n
    spec, xd, god = spec_of(g), dev(x), dev(go)
    tables = table_of(g, half, 3)

    def run():
        buf, out = guarded(n, 3)
        ops.launch("nrhip_hashgrid_bwd_input", spec.c_grid(tables[0]), tables[0], xd, god, n, out)
        return buf

    held(twice(run, "bwd_input"), ref, "bwd_input")
    gid = H.multi_ids(n, 3, 2, False, strays=False)
    mref = np.zeros((n, 3))
    for c in range(3):
        mref[gid == c] = H.input_grad_ref(replace(g, row0=c * g.rows), x[gid == c], go[gid == c])[0]
    ids = dev(gid)

    def run_multi():
        buf, out = guarded(n, 3)
        ops.launch("nrhip_hashgrid_multi_bwd_input", spec.c_grid(tables[0]), ops._ptr_array(tables), 3, ids, xd, god, n, out)
        return buf

    held(twice(run_multi, "multi_bwd_input"), mref, "multi_bwd_input")


# ---------------------------------------------------------------------------------------------------------------------
# atomic scatter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("name,n", FWD_SHAPES)
def test_atomic_scatter(name, n, F):
    case = H.scatter_case(name, F, n)
    g = case.grid
    H.assert_exact_scatter(g, case.x, case.go, partition=False)
    spec, x, go = spec_of(g), dev(case.x), dev(case.go)

    def run():
        buf, gt = guarded(g.rows, g.F, fill=0.0)
        ops.launch("nrhip_hashgrid_bwd", spec.c_grid(gt), x, go, n, gt)
        return buf

    held(twice(run, case.name), H.scatter_ref(g, case.x, case.go), case.name)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R,S,still", [(1, 1, False), (9, 7, False), (1, 64, False), (2, 64, True), (13, 5, False), (257, 1, False)])
def test_atomic_scatter_of_ray_samples(R, S, still, F):
    g = H.Grid(3, 16, 64, 8, F)
    r = H.dense_rays(R, S, 8, seed=R)
    if still:  # two still rays at one point: a run of 64, and equal keys on both sides of the wave boundary 63 | 64
        r.origins[:], r.directions[:] = r.origins[1], 0.0
    pos = H.ray_positions(r)
    go = H.small_grads(R * S, g.width, R)
    H.assert_exact_scatter(g, pos, go, partition=False)
    runs = H.census_runs(g, pos, 64)
    if still:
        assert runs["longest"] == 64 and runs["across"] == g.L * 8
    if (R, S) == (13, 5):
        assert runs["merged"] > 0
    if (R, S) == (257, 1):
        assert runs["groups_without_run"] > 0
    spec, god = spec_of(g), dev(go)
    rays, keep = dense(r)

    def run():
        buf, gt = guarded(g.rows, g.F, fill=0.0)
        ops.launch("nrhip_encode_bwd", spec.c_grid(gt), H.STATIC_SCALE, rays, god, gt)
        return buf

    held(twice(run, "encode_bwd"), H.scatter_ref(g, pos, go), "encode_bwd")


@pytest.mark.parametrize("runs", ("default", "0"))
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", (64, 257))
def test_atomic_scatter_of_several_grids(n, F, runs, switches):
    if runs == "0":
        switches.set("NRHIP_MULTI_BWD_RUNS", "0")
    else:
        switches.unset("NRHIP_MULTI_BWD_RUNS")
    case = H.run_rows_case(F, n)
    g = case.grid
    off = H.row_offsets(case)
    H.assert_exact_scatter(g, case.x, case.go, partition=False, row_offset=off, rows=3 * g.rows)
    s = H.census_runs(g, case.x, 16, key_extra=case.grid_id, live=off >= 0)
    assert s["merged"] > 0 and s["across"] > 0 and s["other_grid"] > 0
    assert (off[[38, 40, 50, 51]] < 0).all() and (off[[37, 39, 41, 49, 52]] >= 0).all()  # strays and the absent grid inside runs
    spec, x, go, ids = spec_of(g), dev(case.x), dev(case.go), dev(case.grid_id)
    ref = H.scatter_ref(g, case.x, case.go, rows=3 * g.rows, row_offset=off)
    assert not ref[2 * g.rows:].any()

    def run():
        buf, flat = guarded(3 * g.rows, g.F, fill=0.0)
        flat[2 * g.rows:] = NAN  # grid 2 wants no gradient: its pointer is NULL and this stretch must stay as it is
        ptrs = torch.tensor([flat.data_ptr(), flat.data_ptr() + g.rows * g.F * 4, 0], dtype=torch.int64, device="cuda")
        ops.launch("nrhip_hashgrid_multi_bwd", spec.c_grid(torch.float32), 3, ids, x, go, n, ptrs)
        return buf

    got = twice(run, case.name)
    ref[2 * g.rows:] = np.nan
    body = got.cpu().numpy()
    assert np.isnan(body[2 * g.rows:]).all(), "rows of the absent grid or the guard row were written"
    held(torch.cat([got[:2 * g.rows], got[-1:]]), ref[:2 * g.rows], case.name)


# ---------------------------------------------------------------------------------------------------------------------
# the partition
# ---------------------------------------------------------------------------------------------------------------------
def workspace(g_c, n, n_slots=None):
    if n_slots is None:
        ws, need = ops._workspace("nrhip_encode_bwd_binned_workspace", g_c, int(n), device="cuda", dtype=torch.uint8)
    else:
        ws, need = ops._workspace("nrhip_hashgrid_multi_bwd_binned_workspace", g_c, int(n_slots), int(n), device="cuda", dtype=torch.uint8)
    assert need > 0
    return ws, need


def binned_given(g: H.Grid, x, go, ref, what, prefills=(NAN, 3.0)):
    """nrhip_hashgrid_bwd_binned: overwrite = 1 over NaN, overwrite = 0 onto a table of 3s"""
    spec, n = spec_of(g), len(x)
    c = spec.c_grid(torch.float32)
    xd, god = dev(x), dev(go)
    ws, need = workspace(c, n)
    for fill in prefills:
        overwrite = 1 if fill != fill else 0

        def run():
            buf, gt = guarded(g.rows, g.F, fill=fill)
            ops.launch("nrhip_hashgrid_bwd_binned", c, xd, god, n, gt, overwrite, ws, need)
            return buf

        held(twice(run, what), ref + (0.0 if overwrite else fill), f"{what}, overwrite {overwrite}")


PAIRS = ("all", "none")


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", (1, 4095, 4096, 4097))
def test_partition_chunk_edges(n, F, pairs, switches):
    switches.set("NRHIP_BIN_PAIRS", pairs)
    case = H.scatter_case("wave", F, n, gmax=2)
    g = case.grid
    H.assert_exact_scatter(g, case.x, case.go, partition=True, prefill=3.0)
    assert H.bin_plan(g, n, pairs == "all")["chunks"] == (2 if n == 4097 else 1)
    binned_given(g, case.x, case.go, H.scatter_ref(g, case.x, case.go), case.name)


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("F", (1, 4))
def test_partition_live_counts(F, pairs, switches):
    """chunks with exactly 1024 live samples (one full pass of the 1024 threads), none at all, 1025, and one"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    n = 3 * H.CHUNK + 7
    live = np.concatenate([np.arange(0, H.CHUNK, 4), 2 * H.CHUNK + np.arange(1025) * 3, [n - 1]])
    g = H.Grid(3, 16, 64, 8, F)
    x = H.lattice_positions(n, 8, 5)
    go = H.sparse_grads(n, g.width, live, 5)
    assert H.live_per_chunk(go) == [1024, 0, 1025, 1]
    H.assert_exact_scatter(g, x[live], go[live], partition=True, prefill=3.0)
    binned_given(g, x, go, H.scatter_ref(g, x[live], go[live]), "live counts")


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("name,L,lo,hi,lg,K,n", [("six", 6, 16, 512, 10, 9, 4097), ("one", 1, 16, 16, 8, 8, 4097),
                                                  ("sliced", 2, 64, 1024, 12, 11, 4097), ("sliced1", 2, 64, 1024, 12, 11, 1)])
@pytest.mark.parametrize("F", (1, 2))
def test_partition_plans(name, L, lo, hi, lg, K, n, F, pairs, switches):
    switches.set("NRHIP_BIN_PAIRS", pairs)
    g = H.Grid(L, lo, hi, lg, F)
    x = H.lattice_positions(n, K, 3)
    go = H.small_grads(n, g.width, 3, gmax=2)
    H.assert_exact_scatter(g, x, go, partition=True, prefill=3.0)
    plan = H.bin_plan(g, n, pairs == "all")
    if name == "six":
        assert plan["lgroups"] == 6
    if name.startswith("sliced"):
        sl = H.census_slices(g, x, plan)
        assert plan["rec_slots"] == 8 and plan["nb"] > 1 and (sl["straddle"] > 0 or n == 1) and (sl["empty"] > 0 or n > 1)
    binned_given(g, x, go, H.scatter_ref(g, x, go), name)


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("L,chunks", [(1, 64), (6, 341), (6, 255)])
def test_partition_many_chunks(L, chunks, pairs, switches):
    """more than 64 chunks: the segment prefix; L = 6 with 342 chunks: a workgroup walks two levels; with 256 chunks the 4 level
    groups the plan wants are bumped to 6, a divisor of L.  Mostly silent samples (whole chunks without a live one) keep the
    reference small."""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    n = chunks * H.CHUNK + 1
    g = H.Grid(L, 16, 16 if L == 1 else 512, 10, 1)
    plan = H.bin_plan(g, n, pairs == "all")
    assert plan["nseg"] == -(-(chunks + 1) // 64) > 1 and plan["lgroups"] == {(1, 64): 1, (6, 341): 3, (6, 255): 6}[L, chunks]
    assert -(-1024 // (chunks + 1)) == {64: 16, 341: 3, 255: 4}[chunks]  # what the plan wants before the clamp and the bump
    rng = np.random.default_rng(chunks)
    live = np.unique(np.concatenate([rng.integers(0, n, 3000), np.arange(70 * H.CHUNK - 40, 70 * H.CHUNK + 40) % n, [0, n - 1]]))
    live = live[(live // H.CHUNK) % 5 != 3]  # every fifth chunk entirely silent
    live = np.unique(np.append(live, n - 1))
    x = H.lattice_positions(n, 9, chunks)
    go = H.sparse_grads(n, g.width, live, chunks)
    H.assert_exact_scatter(g, x[live], go[live], partition=True)
    binned_given(g, x, go, H.scatter_ref(g, x[live], go[live]), "many chunks", prefills=(NAN,))


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("n", ((1 << 15) + 1, 1 << 16))
def test_partition_rounds(n, pairs, switches):
    """two rounds: only the first overwrites; the second holds one sample, or a full round"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    switches.set("NRHIP_BIN_ROUND_LOG2", "15")
    g = H.Grid(3, 16, 64, 8, 2)
    assert H.bin_plan(g, n, pairs == "all", round_log2=15)["rounds"] == 2
    live = np.unique(np.concatenate([np.arange(0, n, 37), [n - 1]]))
    x = H.lattice_positions(n, 8, 9)
    go = H.sparse_grads(n, g.width, live, 9)
    H.assert_exact_scatter(g, x[live], go[live], partition=True, prefill=3.0)
    binned_given(g, x, go, H.scatter_ref(g, x[live], go[live]), "rounds")


@pytest.mark.parametrize("lg,F", [(1, 1), (1, 2), (8, 1), (8, 4)])
def test_partition_of_a_silent_batch(lg, F):
    """no sample sends anything: every slice takes the cnt == 0 fill (2 floats a slice at log2 T = 1, F = 1: the scalar loop)"""
    g = H.Grid(3, 16, 64, lg, F)
    n = 300
    x = H.lattice_positions(n, 8, 1)
    go = H.sparse_grads(n, g.width, [], 1)
    binned_given(g, x, go, np.zeros((g.rows, F)), "silent batch")


@pytest.mark.parametrize("L,F,shift", [(8, 4, 0), (8, 4, 1), (4, 8, 0), (8, 1, 0), (2, 4, 0), (8, 8, 0)])
def test_partition_silent_rows(L, F, shift):
    """rows_are_zero: 32-float rows on and one float off the 16-byte grid, widths 8 and 64; silent rows of +0.0 and -0.0"""
    g = H.Grid(L, 16, 16 << (L - 1), 8, F)
    n = 700
    x = H.lattice_positions(n, 9, L)
    live = np.unique(np.concatenate([np.arange(0, n, 3), np.arange(64, 80), [n - 1]]))
    go = H.sparse_grads(n, g.width, live, L)
    assert (go[13] == 0).all() and np.signbit(go[13]).all() and (go[1] == 0).all() and not np.signbit(go[1]).any()
    H.assert_exact_scatter(g, x[live], go[live], partition=True)
    ref = H.scatter_ref(g, x[live], go[live])
    spec = spec_of(g)
    c = spec.c_grid(torch.float32)
    flat = torch.zeros(n * g.width + 4, device="cuda")
    god = flat[shift:shift + n * g.width]
    god.copy_(dev(go).reshape(-1))
    assert god.data_ptr() % 16 == 4 * shift
    xd = dev(x)
    ws, need = workspace(c, n)

    def run():
        buf, gt = guarded(g.rows, g.F)
        ops.launch("nrhip_hashgrid_bwd_binned", c, xd, god, n, gt, 1, ws, need)
        return buf

    held(twice(run, "silent rows"), ref, "silent rows")


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("F", (1, 4))
@pytest.mark.parametrize("S", (16, 64, 256))
def test_partition_walk_orders(S, F, pairs, switches):
    """a coherent chunk (one origin, near-parallel directions) walked sample-index-major and ray-major, and the same samples as
    bare positions in a shuffled order: the same bits"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    g = H.Grid(3, 16, 64, 8, F)
    R = H.CHUNK // S
    r = H.dense_rays(R, S, 8, 0, mode="fan")
    assert H.coherent_chunk(r, 0, H.CHUNK) == R
    pos = H.ray_positions(r)
    go = H.small_grads(R * S, g.width, S, gmax=2)
    H.assert_exact_scatter(g, pos, go, partition=True, prefill=3.0)
    ref = H.scatter_ref(g, pos, go)
    spec = spec_of(g)
    c = spec.c_grid(torch.float32)
    rays, keep = dense(r)
    god = dev(go)
    ws, need = workspace(c, R * S)
    for transpose in ("1", "0"):
        switches.set("NRHIP_BIN_TRANSPOSE", transpose)

        def run():
            buf, gt = guarded(g.rows, g.F)
            ops.launch("nrhip_encode_bwd_binned", c, H.STATIC_SCALE, rays, god, gt, 1, ws, need)
            return buf

        held(twice(run, f"walk {transpose}"), ref, f"walk {transpose}")
    perm = np.random.default_rng(S).permutation(R * S)
    binned_given(g, pos[perm], go[perm], ref, "shuffled positions")


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("F", (1, 2, 8))
def test_partition_of_ray_samples(F, pairs, switches):
    """dense [R, S] and packed (ragged, with empty rays) sources, fp32 and fp16 gradients"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    g = H.Grid(3, 16, 64, 8, F)
    spec = spec_of(g)
    c = spec.c_grid(torch.float32)
    for r in (H.dense_rays(69, 61, 8, 4), H.packed_rays((0, 3, 0, 0, 17, 1, 0, 64, 5, 0, 33, 65, 2, 0), 8, 4)):
        pos = H.ray_positions(r)
        n = len(pos)
        go = H.small_grads(n, g.width, n, gmax=2)
        H.assert_exact_scatter(g, pos, go, partition=True, prefill=3.0)
        ref = H.scatter_ref(g, pos, go)
        god = dev(go)
        ws, need = workspace(c, n)
        rays, keep = dense(r) if r.ray_of is None else packed(r)
        entry = "nrhip_encode_bwd_binned" + ("" if r.ray_of is None else "_packed")
        mid = (rays,) if r.ray_of is None else (rays, keep[1])
        for fill in (NAN, 3.0):

            def run():
                buf, gt = guarded(g.rows, g.F, fill=fill)
                ops.launch(entry, c, H.STATIC_SCALE, *mid, god, gt, 1 if fill != fill else 0, ws, need)
                return buf

            held(twice(run, entry), ref + (0.0 if fill != fill else fill), entry)


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("F", (1, 4))
def test_partition_fp16_gradients(F, pairs, switches):
    """the _f16 forms: every exact sum is an fp16 number, except two entries beyond fp16's range, which come back +-inf; a
    batch of more than one round is refused and leaves the NaN prefill alone"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    g = H.Grid(3, 16, 64, 8, F)
    spec = spec_of(g)
    c = spec.c_grid(torch.float32)
    r = H.dense_rays(40, 8, 5, 6)
    r.origins[:] = np.random.default_rng(6).integers(-7, 8, (40, 3)) * 2.0  # still rays on the 2^-5 lattice of x
    r.directions[:] = 0
    r.origins[38], r.origins[39] = (4.0, -8.0, 12.0), (-4.0, 8.0, 0.0)  # lattice points of every level: one entry a level
    packed_r = H.Rays(r.origins, r.directions, r.starts.reshape(-1), r.ends.reshape(-1), np.repeat(np.arange(40), 8))
    pos = H.ray_positions(r)
    n = len(pos)
    go = H.small_grads(n, g.width, 6, gmax=2)
    go[38 * 8:39 * 8], go[39 * 8:] = 8192.0, -8192.0  # 8 x 8192 = 65536 > 65504
    H.assert_exact_scatter(g, pos, go, partition=True, out_half=True)
    ref = H.scatter_ref(g, pos, go)
    assert (ref >= 65536).sum() >= F and (ref <= -65536).sum() >= F
    god = dev(go)
    ws, need = workspace(c, n)
    for rr in (r, packed_r):
        rays, keep = dense(rr) if rr.ray_of is None else packed(rr)
        entry = "nrhip_encode_bwd_binned" + ("" if rr.ray_of is None else "_packed") + "_f16"
        mid = (rays,) if rr.ray_of is None else (rays, keep[1])

        def run():
            buf, gt = guarded(g.rows, g.F, dtype=torch.float16)
            ops.launch(entry, c, H.STATIC_SCALE, *mid, god, gt, ws, need)
            return buf

        got = held(twice(run, entry), ref, entry)
        assert np.isinf(got[:-1].astype(np.float64)).sum() == (np.abs(ref) >= 65520).sum()  # (fp16 rounds 65520 up to inf)
    # a silent batch: every slice takes the fp16 cnt == 0 fill
    silent = torch.zeros_like(god)
    rays, keep = dense(r)

    def run_silent():
        buf, gt = guarded(g.rows, g.F, dtype=torch.float16)
        ops.launch("nrhip_encode_bwd_binned_f16", c, H.STATIC_SCALE, rays, silent, gt, ws, need)
        return buf

    held(twice(run_silent, "silent f16"), np.zeros((g.rows, F)), "silent f16")
    # more than one round
    switches.set("NRHIP_BIN_ROUND_LOG2", "15")
    R2 = (1 << 15) // 8 + 1
    r2 = H.Rays(np.tile(r.origins[:1], (R2, 1)), np.zeros((R2, 3), np.float32), np.tile(r.starts[:1], (R2, 1)), np.tile(r.ends[:1], (R2, 1)))
    rays, keep = dense(r2)
    god2 = torch.ones((R2 * 8, g.width), device="cuda")
    ws, need = workspace(c, R2 * 8)
    buf, gt = guarded(g.rows, g.F, dtype=torch.float16)
    with pytest.raises(_lib.NeuradHipError, match="one round"):
        ops.launch("nrhip_encode_bwd_binned_f16", c, H.STATIC_SCALE, rays, god2, gt, ws, need)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("F", (1, 4))
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("empty_slot", (False, True), ids=("", "empty-slot"))
def test_partition_of_several_grids(empty_slot, half, F, pairs, switches):
    """5 grids, 3 slots: grids 1 and 3 want no gradient (slot_of < 0), ids -1 and n_grids send nothing; every element of the
    [slot][L T][F] block is written"""
    switches.set("NRHIP_BIN_PAIRS", pairs)
    n, n_grids, n_slots = 4097, 5, 3
    g = H.Grid(3, 16, 64, 8, F)
    K = 5 if half else 8
    x = H.lattice_positions(n, K, 8)
    gid = H.multi_ids(n, n_grids, 8, True, strays=True)
    if empty_slot:  # no sample of grid 4: every slice of slot 1, in the middle of the block, takes the cnt == 0 fill
        gid[gid == 4] = 0
    slot_of = np.array([2, -1, 0, -3, 1], np.int32)
    case = H.Case("multi", g, x, grid_id=gid, n_grids=n_grids)
    off = H.row_offsets(case, slot_of)
    assert (off < 0).sum() > 100 and len(np.unique(off)) == (3 if empty_slot else 4)
    live = np.unique(np.concatenate([np.arange(0, n, 5 if half else 1), [n - 1]]))
    go = H.sparse_grads(n, g.width, live, 8, gmax=1 if half else 2)
    H.assert_exact_scatter(g, x, go, partition=True, row_offset=off, rows=n_slots * g.rows, out_half=half)
    ref = H.scatter_ref(g, x, go, rows=n_slots * g.rows, row_offset=off)
    spec = spec_of(g)
    c = spec.c_grid(torch.float32)
    xd, god, ids, slots = dev(x), dev(go), dev(gid), dev(slot_of)
    ws, need = workspace(c, n, n_slots)

    def run():
        buf, block = guarded(n_slots * g.rows, g.F, dtype=torch.float16 if half else torch.float32)
        ops.launch("nrhip_hashgrid_multi_bwd_binned", c, n_grids, ids, slots, n_slots, xd, god, n, block, 1 if half else 0, ws, need)
        return buf

    held(twice(run, "multi binned"), ref, "multi binned")


# ---------------------------------------------------------------------------------------------------------------------
# the two host refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_lookups_refuse_a_table_off_the_16_byte_grid_and_a_two_entry_level():
    g = H.Grid(3, 16, 64, 8, 1)
    spec = spec_of(g)
    flat = torch.zeros(g.rows + 4, device="cuda")
    x = dev(H.lattice_positions(8, 8, 0))
    buf, out = guarded(8, g.width)
    c = spec.c_grid(torch.float32)
    with pytest.raises(_lib.NeuradHipError, match="16-byte aligned"):
        ops.launch("nrhip_hashgrid_fwd", c, flat[1:1 + g.rows], x, 8, out)
    tiny = spec_of(H.Grid(3, 16, 64, 1, 1)).c_grid(torch.float32)
    with pytest.raises(_lib.NeuradHipError, match="log2_table_size >= 2"):
        ops.launch("nrhip_hashgrid_fwd", tiny, flat, x, 8, out)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    half = torch.zeros(6, 1, device="cuda", dtype=torch.float16)  # fp16: 2-entry levels are whole 4-byte pairs
    ops.launch("nrhip_hashgrid_fwd", spec_of(H.Grid(3, 16, 64, 1, 1)).c_grid(half), half, x, 8, out)
    torch.cuda.synchronize()
    assert (buf[:8] == 0).all()
