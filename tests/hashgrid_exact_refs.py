"""The exact lattice family of the standalone hash-grid kernels (csrc/hashgrid.hip, csrc/encode_bwd_binned.hip, the dispatch
side of csrc/hashgrid_dx.hip): cases, int64 / float64 references and censuses, shared by test_hashgrid_exact_refs_host.py
(CPU) and test_gpu_hashgrid_exact.py (device).

Why one right answer per element exists.  Every scaling is an integer (floor(min_res * g^l)); positions are dyadic
(x = m / 2^K), so x * scal, its floor and the offset o = x * scal - floor are exact in fp32 and o is a multiple of
2^-(K - v), v = the power of two in scal.  Table values and incoming gradients are small integers.  Every corner term
w_k * value is then an integer number of one QUANTUM q (a power of two), and wherever the sum of the absolute terms of an
output stays below 2^24 q, every partial sum in ANY order, with or without fma contraction, is an integer below 2^24 quanta:
exactly representable in fp32.  The lerp tree (common.h lerp_corners), the corner weights, the DPP / shuffle run merges, the
fp32 atomics and the partition's 64-bit fixed-point image (quantum 2^-sh, far finer) then all give the SAME bits, those of
the float64 sum.  ``assert_exact`` checks exactly these premises, per case, in float64.

The reference takes its corner rows and offsets from the oracle (``O.hashgrid_corner_indices``) and sums in float64; it
shares no code with the kernels.  ``mutated`` restates the reference with one defect (a corner slot swapped, floor for ceil,
o for 1 - o, a sample or a term lost or doubled, another level's scaling); the host tests show every case sees every defect.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import neurad_oracle as O

f32, f64 = np.float32, np.float64
LIMIT = 2.0 ** 24
PRIME_ROW = 2654435761
CORNERS = ("ccc", "cfc", "ffc", "fcc", "ccf", "cff", "fff", "fcf")  # encodings.py:437-444: (x, y, z) ceil | floor
PAIR_F, PAIR_C = (3, 2, 7, 6), (0, 1, 4, 5)  # (floor x, ceil x) slots of the pairs (y, z) = cc, fc, cf, ff
STATIC_SCALE = 16.0
CHUNK = 4096  # kSamplesPerBlock of csrc/encode_bwd_binned.hip
SEG_CHUNKS = 64


# ------------------------------------------------------------------------------------------------------------------
# grids and tables
# ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Grid:
    L: int
    min_res: int
    max_res: int
    lg: int
    F: int
    row0: int = 0  # first row of this grid's table in the (endless) formula table: the grids of one multi-grid call differ in it

    @property
    def T(self):
        return 1 << self.lg

    @property
    def rows(self):
        return self.L << self.lg

    @property
    def scal(self):
        return O.hash_scalings(self.L, self.min_res, self.max_res)

    @property
    def width(self):
        return self.L * self.F


def table_formula(row, f, F):
    """the table value of feature ``f`` of row ``row``: a fixed small integer in [-64, 64) of the ELEMENT number row * F + f
    (F = 1: of the row).  Works on numpy and torch int64 alike (the 4 GiB table is filled on the device, in chunks).
    Consecutive elements step by 0.618 * 128 = 79 (mod 128): the four rows of an aligned 4-block always differ."""
    return ((((row * F + f) * PRIME_ROW) % (1 << 32)) >> 25) - 64


def table_at(grid: Grid, rows) -> np.ndarray:
    """float64 [..., F]: the table's values at ``rows`` (the reference never holds a whole table: the largest has 2^30 elements)"""
    rows = np.asarray(rows, np.int64)[..., None] + grid.row0
    return table_formula(rows, np.arange(grid.F, dtype=np.int64), grid.F).astype(f64)


def table_values(grid: Grid) -> np.ndarray:
    """int64 [rows, F]; exact in fp32 and fp16"""
    row = np.arange(grid.rows, dtype=np.int64)[:, None] + grid.row0
    return table_formula(row, np.arange(grid.F, dtype=np.int64)[None, :], grid.F)


# ------------------------------------------------------------------------------------------------------------------
# positions
# ------------------------------------------------------------------------------------------------------------------
def edge_positions(K: int) -> np.ndarray:
    """the rows every family of positions starts with: exactly 0 and 1 on each axis, the last lattice point below 1, lattice
    on one, two and three axes (0, 1/2 and 1 are lattice points of every level with an even scaling, 0 and 1 of every
    level), coordinates in [-1, 0) and (1, 2]"""
    e, h, a, b = (2.0 ** K - 1) / 2.0 ** K, 0.5, 1 / 2.0 ** K, 3 / 2.0 ** K
    return np.array([
        [0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 1], [0, 0, 1], [1, 1, 0],
        [e, e, e], [e, a, b], [a, e, 0], [1, b, e],
        [h, a, b], [a, h, e], [b, e, h], [h, h, a], [a, h, h], [h, b, h], [h, h, h], [0, h, 1],
        [-a, a, b], [a, -h, b], [b, a, -1], [-e, -b, -a], [1 + a, b, a], [a, 2, b], [b, a, 1 + e], [2, 1 + h, -1],
    ], f64)


def lattice_positions(n: int, K: int, seed: int, edges: bool = True) -> np.ndarray:
    """fp32 [n, 3] on the lattice m / 2^K: the edge rows first (as many as fit, never the last row), then uniform draws that
    are lattice points of NO level on any axis (odd m: all 8 corners distinct cells)"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << (K - 1), (n, 3)) * 2 + 1
    x = m / 2.0 ** K
    if edges and n > 1:
        e = edge_positions(K)[: n - 1]
        x[: len(e)] = e
    return x.astype(f32)


def small_grads(n: int, width: int, seed: int, gmax: int = 8, silent: bool = True) -> np.ndarray:
    """fp32 [n, width] integers in [-gmax, gmax]; rows 3 (all +0.0) and 5 (all -0.0) are silent; the last row never is"""
    rng = np.random.default_rng(seed + 77)
    g = rng.integers(-gmax, gmax + 1, (n, width)).astype(f32)
    g[-1, 0] = gmax
    if silent and n > 6:
        g[3] = 0.0
        g[5] = -0.0
    return g


def sparse_grads(n: int, width: int, live, seed: int, gmax: int = 2) -> np.ndarray:
    """fp32 [n, width]: rows ``live`` hold integers in [-gmax, gmax] with a non-zero first column, every other row is silent
    (+0.0, every 7th silent row -0.0)"""
    rng = np.random.default_rng(seed + 99)
    g = np.zeros((n, width), f32)
    g[6::7] = -0.0
    live = np.asarray(live, np.int64)
    v = rng.integers(-gmax, gmax + 1, (len(live), width)).astype(f32)
    v[:, 0] = np.where(v[:, 0] == 0, 1, v[:, 0])
    g[live] = v
    return g


# ------------------------------------------------------------------------------------------------------------------
# the reference: corners from the oracle, everything else float64
# ------------------------------------------------------------------------------------------------------------------
def own_indices(x: np.ndarray, scal: np.ndarray, T: int, floor_for_ceil: Optional[int] = None):
    """the hash restated on int64 (for the mutants, and held to the oracle's by the host tests): idx [N, L, 8] with the level
    offset, o [N, L, 3] float64"""
    s = x.astype(f64)[:, None, :] * scal.astype(f64)[None, :, None]
    fl, ce = np.floor(s).astype(np.int64), np.ceil(s).astype(np.int64)
    if floor_for_ceil is not None:
        ce = ce.copy()
        ce[..., floor_for_ceil] = fl[..., floor_for_ceil]
    lo = (np.arange(len(scal), dtype=np.int64) * T)[None, :]
    idx = []
    for c in CORNERS:
        p = [ce[..., a] if c[a] == "c" else fl[..., a] for a in range(3)]
        idx.append(((p[0] ^ (p[1] * 2654435761) ^ (p[2] * 805459861)) % T) + lo)
    return np.stack(idx, -1), s - fl


def corner_terms(grid: Grid, x: np.ndarray, mutate=None):
    """-> (idx [N, L, 8] int64 rows, w [N, L, 8] float64 corner weights).  Unmutated: rows and offsets are the ORACLE's, and
    the offsets are shown to be exact (fp32 product == float64 product)."""
    scal = grid.scal
    kind = mutate[0] if mutate else None
    if kind == "level":  # another level's scaling
        scal = np.roll(scal, 1) if grid.L > 1 else scal + f32(1)
    if kind in ("floor_for_ceil", "level"):
        idx, o = own_indices(x, scal, grid.T, mutate[1] if kind == "floor_for_ceil" else None)
    else:
        idx, o32 = O.hashgrid_corner_indices(x, scal, grid.T)
        s = x.astype(f64)[:, None, :] * scal.astype(f64)[None, :, None]
        o = s - np.floor(s)
        assert (o == o32).all(), "x * scal is not exact in fp32: the lattice is too fine for this grid"
    if kind == "flip_o":
        o = o.copy()
        o[..., mutate[1]] = 1.0 - o[..., mutate[1]]
    w = np.empty(idx.shape, f64)
    for k, c in enumerate(CORNERS):
        w[..., k] = np.prod([o[..., a] if c[a] == "c" else 1.0 - o[..., a] for a in range(3)], 0)
    if kind == "swap":
        idx = idx.copy()
        idx[..., [mutate[1], mutate[2]]] = idx[..., [mutate[2], mutate[1]]]
    return idx, w


def _first_nonzero(t):
    nz = np.argwhere(t.reshape(t.shape[0], t.shape[1], 8, -1).any(-1))
    return tuple(nz[len(nz) // 2])


def forward_terms(grid: Grid, x, mutate=None):
    """the 8 corner terms of every output element, float64 [N, L, 8, F]"""
    idx, w = corner_terms(grid, x, mutate)
    return w[..., None] * table_at(grid, idx)


def forward_ref(grid: Grid, x, mutate=None) -> np.ndarray:
    """float64 [N, L * F].  Sample-level mutants: the last sample's row never written (NaN, the prefill), one corner term of
    one element lost, one sample's terms added twice."""
    t = forward_terms(grid, x, mutate)
    kind = mutate[0] if mutate else None
    if kind == "drop_term":
        t[_first_nonzero(t)] = 0.0
    out = t.sum(2)
    if kind == "dup_sample":
        out[_first_nonzero(t)[0]] *= 2.0
    if kind == "drop_last":
        out[-1] = np.nan
    return out.reshape(len(x), grid.width)


def scatter_terms(grid: Grid, x, go, mutate=None):
    """-> (idx [N, L, 8], terms float64 [N, L, 8, F]) of the table gradient"""
    idx, w = corner_terms(grid, x, mutate)
    return idx, w[..., None] * np.asarray(go, f64).reshape(len(x), grid.L, 1, grid.F)


def scatter_ref(grid: Grid, x, go, mutate=None, rows: Optional[int] = None, row_offset=None) -> np.ndarray:
    """float64 [rows, F]: the table gradient.  row_offset [N] (multi-grid): first row of each sample's table in the block,
    < 0: the sample sends nothing."""
    if mutate is None and row_offset is None and len(x) > 4 * CHUNK:  # a large, mostly silent batch: the live rows only
        live = np.flatnonzero((np.asarray(go) != 0).any(1))
        x, go = x[live], np.asarray(go)[live]
    idx, t = scatter_terms(grid, x, go, mutate)
    kind = mutate[0] if mutate else None
    keep = np.ones(len(x), bool)
    if row_offset is not None:
        keep &= np.asarray(row_offset) >= 0
        idx = idx + np.maximum(np.asarray(row_offset, np.int64), 0)[:, None, None]
    if kind == "drop_last":
        keep[np.flatnonzero(keep & t.reshape(len(x), -1).any(1))[-1]] = False
    if kind == "drop_term":
        t[_first_nonzero(t * keep[:, None, None, None])] = 0.0
    if kind == "dup_sample":
        i = _first_nonzero(t * keep[:, None, None, None])[0]
        idx, t, keep = np.concatenate([idx, idx[i:i + 1]]), np.concatenate([t, t[i:i + 1]]), np.append(keep, True)
    out = np.zeros((grid.rows if rows is None else rows, grid.F), f64)
    np.add.at(out, idx[keep].reshape(-1), t[keep].reshape(-1, grid.F))
    return out


def input_grad_ref(grid: Grid, x, go):
    """dL/dx of the lookup (floor / ceil carry no gradient): -> (float64 [N, 3], the sum of its absolute elementary terms
    [N, 3], their quantum).  d/dx_a = sum_l scal_l sum_q go sum_k value_k s_a(k) prod_{b != a} w_b(k), s = +1 ceil, -1 floor."""
    idx, _ = corner_terms(grid, x)
    s = x.astype(f64)[:, None, :] * grid.scal.astype(f64)[None, :, None]
    o = s - np.floor(s)
    v = table_at(grid, idx)  # [N, L, 8, F]
    g = np.asarray(go, f64).reshape(len(x), grid.L, 1, grid.F)
    out, mag, terms = np.zeros((len(x), 3), f64), np.zeros((len(x), 3), f64), []
    for a in range(3):
        d = np.empty(idx.shape, f64)
        for k, c in enumerate(CORNERS):
            d[..., k] = (1.0 if c[a] == "c" else -1.0) * np.prod(
                [o[..., b] if c[b] == "c" else 1.0 - o[..., b] for b in range(3) if b != a], 0)
        t = grid.scal.astype(f64)[None, :, None, None] * g * v * d[..., None]
        out[:, a], mag[:, a] = t.sum((1, 2, 3)), np.abs(t).sum((1, 2, 3))
        terms.append(t)
    return out, mag, quantum(np.stack(terms))


# ------------------------------------------------------------------------------------------------------------------
# exactness
# ------------------------------------------------------------------------------------------------------------------
def quantum(t) -> float:
    """the largest power of two that divides every term (1.0 when all are zero)"""
    t = np.abs(np.asarray(t, f64))
    t = t[t != 0]
    if t.size == 0:
        return 1.0
    m, e = np.frexp(t)  # t = m * 2^e, m in [0.5, 1) with at most 53 bits
    mant = (m * 2.0 ** 53).astype(np.int64)
    tz = np.int64(53) - np.log2((mant & -mant).astype(f64)).astype(np.int64)  # significant bits of m
    return float(2.0 ** int((e - tz).min()))


def assert_sums_exact(terms, sums_abs, what: str) -> float:
    """every term a multiple of the quantum, every sum of absolute terms below 2^24 quanta -> the quantum"""
    q = quantum(terms)
    r = np.asarray(terms, f64) / q
    assert (r == np.rint(r)).all(), what
    assert float(np.max(sums_abs, initial=0.0)) < LIMIT * q, (what, float(np.max(sums_abs)), q)
    return q


def fixed_point_shift(vmax: float, count: int, pair: bool) -> int:
    """bin_reduce_kernel's own formula: sh = 61 - hb - (e + 1), hb = (PAIR ? 33 : 32) - clz(count), e = exponent(vmax)"""
    e = int(np.frexp(f32(vmax))[1]) - 1
    hb = (33 if pair else 32) - (32 - int(count).bit_length())
    return 61 - hb - (e + 1)


def assert_exact_forward(grid: Grid, x) -> float:
    """(table values are integers in [-64, 64): exact in fp32 and in fp16 storage alike).  An output element belongs to one
    level, so every level has its own quantum; -> the finest."""
    t = forward_terms(grid, x)
    return min(assert_sums_exact(t[:, l], np.abs(t[:, l]).sum(1), f"forward, level {l}") for l in range(grid.L))


def assert_exact_scatter(grid: Grid, x, go, partition: bool, row_offset=None, rows=None, out_half=False, prefill=0.0) -> float:
    """the scatter premises; partition: also quantum >= 2^-sh for BOTH pair settings, with the level's largest possible record
    (a whole entry's absolute sum: every run merge stays below it) and every record of the level in one slice"""
    idx, t = scatter_terms(grid, x, go)
    n = len(x)
    keep = np.ones(n, bool) if row_offset is None else np.asarray(row_offset) >= 0
    if row_offset is not None:
        idx = idx + np.maximum(np.asarray(row_offset, np.int64), 0)[:, None, None]
    sums = np.zeros((grid.rows if rows is None else rows, grid.F), f64)
    np.add.at(sums, idx[keep].reshape(-1), np.abs(t[keep]).reshape(-1, grid.F))
    level_of = (np.arange(len(sums)) % grid.rows) >> grid.lg  # a table entry belongs to one level: a quantum per level
    q = 1.0
    for l in range(grid.L):
        ql = assert_sums_exact(t[keep][:, l], sums[level_of == l] + abs(prefill), f"scatter, level {l}")
        q = min(q, ql)
        if partition and sums[level_of == l].max() > 0:
            for pair in (False, True):
                sh = fixed_point_shift(sums[level_of == l].max(), 8 * n, pair)
                assert ql >= 2.0 ** -sh, (ql, sh)
    if out_half:  # every exact sum an fp16 number (integers up to 2048) or beyond fp16's largest finite (-> inf)
        tot = np.zeros_like(sums)
        np.add.at(tot, idx[keep].reshape(-1), t[keep].reshape(-1, grid.F))
        with np.errstate(over="ignore"):
            ok = (tot == tot.astype(np.float16).astype(f64)) | (np.abs(tot) >= 65520.0)
        assert ok.all()
    return q


# ------------------------------------------------------------------------------------------------------------------
# ray sources: dyadic origins, directions and interval ends, static_scale 16, pixel_area 0 (std = 0, rescale weight rcp(1))
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Rays:
    origins: np.ndarray  # [R, 3] fp32
    directions: np.ndarray  # [R, 3] fp32
    starts: np.ndarray  # dense [R, S] | packed [M]
    ends: np.ndarray
    ray_of: Optional[np.ndarray] = None  # packed: [M] int64, the march's ray_indices (sorted, rays may be absent)

    @property
    def area(self):
        return np.zeros(len(self.origins), f32)


def ray_positions(r: Rays) -> np.ndarray:
    """fp32 [N, 3] contracted positions by the oracle (fp32, op for op the reference's), shown EXACT: the same chain in float64
    gives the same numbers, so no step rounds and no order of operations matters."""
    st, en = np.atleast_2d(r.starts), np.atleast_2d(r.ends)
    if r.ray_of is None:
        o, d, a = r.origins, r.directions, r.area
    else:
        o, d, a = r.origins[r.ray_of], r.directions[r.ray_of], r.area[r.ray_of]
        st, en = st.reshape(-1, 1), en.reshape(-1, 1)
    mean, std = O.fast_isotropic_gaussian(o, d, a, st, en)
    pos, cstd = O.contract_gaussian(mean, std, STATIC_SCALE)
    assert (cstd == 0).all()
    t = st.astype(f64) + (en.astype(f64) - st.astype(f64)) / 2.0
    u = (o.astype(f64)[:, None, :] + d.astype(f64)[:, None, :] * t[..., None]) / STATIC_SCALE
    mag = np.abs(u).max(-1, keepdims=True)
    cm = np.maximum(mag, 1.0)
    c = np.where(mag < 1, u, (2.0 - 1.0 / cm) * (u / cm))
    p64 = (c + 2.0) / 4.0
    assert (p64 == pos).all(), "a ray sample's contracted position is not exact in fp32"
    return pos.reshape(-1, 3)


CONTRACTED_U = np.array([  # |u|_inf exactly 2 and 4 (2 - 1/m exact), with ties of the inf-norm; 1 (the boundary itself)
    [2, 0.5, -1], [4, 1, -2], [-2, 2, 0.25], [-4, 4, 2], [2, -2, 2], [1, -4, 4], [0.5, -2, 1.5], [4, 4, -4],
    [1, 0.25, -0.5], [-1, 1, 0.5], [0.75, -0.25, 1]], f64)


def dense_rays(R: int, S: int, K: int, seed: int, mode: str = "march") -> Rays:
    """[R, S] samples.  Sample s of a ray sits at t = tj (starts tj - 1, ends tj + 1), u = u0 + du * tj.
    mode "march": u0 on the 2^-(K-2) lattice inside (-1, 1), du one or two lattice steps on some axes, tj = s // rep: runs of
    equal and of neighbouring positions.  The first rays are overwritten with still rays (du = 0) at CONTRACTED_U.
    mode "fan": one origin, near-parallel dyadic directions (a camera patch's pixel row)."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -(K - 2)  # the lattice step of u = 4 x - 2
    if mode == "fan":  # u = (-1/2 + j / 32, -1/4 + a j / 1024, 1/8), j = s // rep: 16 stations along each ray
        o = np.tile(np.array([[-8.0, -4.0, 2.0]]), (R, 1))
        d = np.stack([np.ones(R), (np.arange(R) % 4) / 32.0, np.zeros(R)], -1)
        tj = np.tile((np.arange(S) // max(S // 16, 1))[None, :] * 0.5, (R, 1))
    else:
        u0 = (rng.integers(-(1 << (K - 5)), 1 << (K - 5), (R, 3)) * 2 + 1) * q  # odd lattice points, |u0| < 1/4
        du = rng.integers(0, 2, (R, 3)) * q
        o, d = u0 * STATIC_SCALE, du * STATIC_SCALE
        rep = rng.integers(2, 6, (R, 1))
        tj = (np.arange(S)[None, :] // rep).astype(f64)  # at most 32 steps for S <= 65: |u| < 1
        k = min(len(CONTRACTED_U), R // 2)
        o[:k], d[:k] = CONTRACTED_U[:k] * STATIC_SCALE, 0.0
    return Rays(o.astype(f32), d.astype(f32), (tj - 1).astype(f32), (tj + 1).astype(f32))


def packed_rays(counts, K: int, seed: int) -> Rays:
    """ragged segments (counts per ray, zeros allowed) of the same march rays, flattened in ray order: ray_of is the march's
    ray_indices (ray r's samples contiguous, rays in increasing order)"""
    counts = np.asarray(counts, np.int64)
    S = int(counts.max())
    d = dense_rays(len(counts), S, K, seed)
    sel = np.arange(S)[None, :] < counts[:, None]
    return Rays(d.origins, d.directions, d.starts[sel], d.ends[sel], np.repeat(np.arange(len(counts)), counts))


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    grid: Grid
    x: np.ndarray  # fp32 [N, 3]: the positions (of ray sources: their contracted positions)
    go: Optional[np.ndarray] = None  # fp32 [N, L * F]
    rays: Optional[Rays] = None
    grid_id: Optional[np.ndarray] = None  # multi-grid: int32 [N]
    n_grids: int = 0
    slot_of: Optional[np.ndarray] = None  # multi-grid partition: int32 [n_grids]
    n_slots: int = 0
    absent: tuple = ()  # multi-grid atomics: grids whose gradient pointer is NULL
    K: int = 0
    extra: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.x)


FWD_GRIDS = {  # (L, min, max, log2 T, K) by name; F is the test's parameter
    "wave": (3, 16, 64, 8, 8),  # n L = 255, 256, 257: a sample's levels straddle a wave and a workgroup
    "block1": (3, 16, 64, 2, 8),  # one aligned 4-block per level
    "block2": (3, 16, 64, 3, 8),
    "odd": (2, 5, 11, 2, 5),  # odd scalings: only 0 and 1 are lattice points
    "mixed": (2, 12, 40, 6, 6),
    "one": (1, 16, 16, 8, 8),  # L = 1: n threads
    "four": (4, 16, 128, 10, 9),
    "wave9": (3, 16, 64, 8, 9),  # (K = 10 puts |value| = 64 at a lattice point exactly ON the bound of 2^24 quanta of 2^-18)
    "fine": (2, 4096, 8192, 19, 5),  # hashed levels: index bits above 16, the uint32 wrap of the prime products
}


def forward_case(name: str, F: int, n: int, seed: int = 0) -> Case:
    L, lo, hi, lg, K = FWD_GRIDS[name]
    if name == "fine":  # x * 8192 = m * 2^(13 - K): every x a lattice point; shift the lattice by an odd 2^-16 step instead
        rng = np.random.default_rng(seed)
        m = rng.integers(0, 1 << 11, (n, 3)) * 32 + rng.integers(1, 8, (n, 3)) * 4 + 2  # x = m / 2^16, o = multiples of 1/8
        return Case(f"fine-F{F}-n{n}", Grid(L, lo, hi, lg, F), (m / 2.0 ** 16).astype(f32), K=16)
    return Case(f"{name}-F{F}-n{n}", Grid(L, lo, hi, lg, F), lattice_positions(n, K, seed), K=K)


def scatter_case(name: str, F: int, n: int, seed: int = 0, gmax: int = 8) -> Case:
    c = forward_case(name, F, n, seed)
    c.go = small_grads(n, c.grid.width, seed, gmax)
    return c


def multi_ids(n: int, n_grids: int, seed: int, sorted_ids: bool, strays: bool) -> np.ndarray:
    rng = np.random.default_rng(seed + 5)
    g = rng.integers(0, n_grids, n).astype(np.int32)
    if sorted_ids:
        g = np.sort(g)
    if strays and n > 40:
        g[[9, 21]] = -1, n_grids  # no such grid
    return g


def run_rows_case(F: int, n: int, n_grids: int = 3, seed: int = 0) -> Case:
    """multi-grid rows for the 16-lane DPP runs: rows in blocks of equal position (equal entries in neighbouring lanes).
    Rows 12..19: one position, one grid: a run across lanes 15 | 16.  Rows 24..31: one position, ids 0 0 0 1 1 0 0 2: equal
    entries of DIFFERENT grids next to each other.  Rows 36..43: a run with ids -1 and n_grids in the middle.  Rows 48..55: a
    run through grid 2, whose gradient pointer is absent.  The rest: runs of random length, ids sorted within."""
    L, lo, hi, lg, K = FWD_GRIDS["wave"]
    grid = Grid(L, lo, hi, lg, F)
    rng = np.random.default_rng(seed)
    base = lattice_positions(n, K, seed, edges=False)
    rep = np.repeat(np.arange(n), rng.integers(1, 6, n))[:n]
    x = base[rep]
    gid = rng.integers(0, 2, n).astype(np.int32)[rep]
    if n >= 64:
        for a, ids in ((12, [1] * 8), (24, [0, 0, 0, 1, 1, 0, 0, 2]), (36, [0, 0, -1, 0, n_grids, 0, 0, 0]), (48, [1, 1, 2, 2, 1, 1, 2, 1])):
            x[a:a + 8] = base[a]
            gid[a:a + 8] = ids
    c = Case(f"runs-F{F}-n{n}", grid, x, small_grads(n, grid.width, seed, silent=False), grid_id=gid, n_grids=n_grids, absent=(2,), K=K)
    return c


def row_offsets(case: Case, slot_of=None) -> np.ndarray:
    """first row of each sample's gradient table in a [slot][L * T][F] block, -1: the sample sends nothing"""
    g = case.grid_id.astype(np.int64)
    ok = (g >= 0) & (g < case.n_grids)
    slot = np.where(ok, np.asarray(slot_of if slot_of is not None else np.arange(case.n_grids), np.int64)[np.where(ok, g, 0)], -1)
    if slot_of is None:
        slot = np.where(np.isin(g, case.absent), -1, slot)
    return np.where(slot >= 0, slot * case.grid.rows, -1)


# ------------------------------------------------------------------------------------------------------------------
# the partition's plan, restated (make_plan of csrc/encode_bwd_binned.hip) -- for the censuses only
# ------------------------------------------------------------------------------------------------------------------
def bin_plan(grid: Grid, n_total: int, pairs: Optional[bool] = None, n_slots: int = 1, round_log2: int = 23) -> dict:
    n = min(n_total, 1 << round_log2)
    log2TS = min(14 - (grid.F.bit_length() - 1), grid.lg)
    while ((grid.L * n_slots) << (grid.lg - log2TS)) < 512 and log2TS > 9:
        log2TS -= 1
    nb = (1 << (grid.lg - log2TS)) * n_slots
    chunks = -(-n // CHUNK)
    lgr = min(max(-(-1024 // chunks), 1), grid.L)
    while grid.L % lgr:
        lgr += 1
    pair = (grid.F == 1) if pairs is None else pairs
    rec_slots = 4 if pair and float(grid.scal.max()) + 2.0 < (1 << log2TS) else 8
    return dict(log2TS=log2TS, nb=nb, chunks=chunks, lgroups=lgr, pair=pair, rec_slots=rec_slots,
                rounds=-(-n_total // (1 << round_log2)), nseg=-(-chunks // SEG_CHUNKS))


# ------------------------------------------------------------------------------------------------------------------
# censuses: how many (sample, level) pairs -- or waves, chunks, slices -- reach a branch
# ------------------------------------------------------------------------------------------------------------------
def _masked(grid: Grid, x):
    idx, _ = O.hashgrid_corner_indices(x, grid.scal, grid.T)
    return idx, idx & (grid.T - 1)


def census_paired(grid: Grid, x, half: bool) -> dict:
    """load_corners_f1 (F = 1, thread = (sample, level), level fastest).  xm = masked floor-x row ^ ceil-x row; `same` (one
    aligned load serves both corners) where xm >> 2 == 0 (fp16: >> 1).  -> pairs per class, pairs per branch, the number of
    WAVES that hold every class at once, and the (rf & 3, rc & 3) combinations (fp16: & 1) seen under `same`."""
    rows, m = _masked(grid, x)
    xm = (m[..., 3] ^ m[..., 0]).reshape(-1)
    sh = 1 if half else 2
    same = (xm >> sh) == 0
    classes = (0, 1) if half else (0, 1, 3)
    wave = np.arange(xm.size) // 64
    per_wave = [set(np.unique(np.where(same[wave == w], xm[wave == w], -1))) for w in range(wave.max() + 1)]
    need = set(classes) | {-1}
    lo = 1 if half else 3
    combos = set()
    for f, c in zip(PAIR_F, PAIR_C):
        rf, rc = rows[..., f].reshape(-1)[same] & lo, rows[..., c].reshape(-1)[same] & lo
        combos |= set(zip(rf.tolist(), rc.tolist()))
    return dict(classes={c: int((xm == c).sum()) for c in classes}, other=int((~same).sum()), same=int(same.sum()),
                full_waves=sum(need <= s for s in per_wave), combos=combos)


def admitted_combos(grid: Grid, half: bool) -> set:
    """every (rf & 3, rc & 3) that `same` admits on this grid: rf ^ rc in {0, 1, 3} (fp16: (rf & 1, rc & 1), xor in {0, 1}),
    limited to the xors a T-entry level can produce (floor ^ ceil = 2^k - 1, masked)"""
    lo = 1 if half else 3
    xors = {v & (grid.T - 1) & lo for v in ((0, 1) if half else (0, 1, 3))}
    return {(a, a ^ v) for a in range(lo + 1) for v in xors}


def census_positions(grid: Grid, x) -> dict:
    """lattice on 1 / 2 / 3 axes (offset exactly 0), coordinates outside [0, 1], rows with bits above 16, corner sets with
    8 distinct rows"""
    rows, m = _masked(grid, x)
    s = x.astype(f64)[:, None, :] * grid.scal.astype(f64)[None, :, None]
    lat = (s == np.floor(s)).sum(-1)
    return dict(lattice={k: int((lat == k).sum()) for k in (1, 2, 3)}, below=int((x < 0).any(1).sum()), above=int((x > 1).any(1).sum()),
                zero=int((x == 0).any(1).sum()), one=int((x == 1).any(1).sum()), high_bits=int((m >> 16 != 0).sum()),
                distinct8=int((np.sort(m, -1)[..., 1:] != np.sort(m, -1)[..., :-1]).all(-1).sum()),
                offset_2g=int(((rows * (4 * grid.F)) >= 2 ** 31).sum()))


def census_runs(grid: Grid, x, width: int, key_extra=None, live=None) -> dict:
    """runs of equal corner rows in neighbouring lanes (one lane a sample, `width` lanes a merge group: 64 for
    encode_bwd_runs_kernel, 16 for the DPP rows).  -> merges inside a group, equal neighbours ACROSS a group boundary (which
    must not merge), the longest run, (full group, level, corner) triples without any run (every lane a head: the merge is
    skipped), and equal rows with
    different ``key_extra`` (grid) in neighbouring lanes."""
    _, m = _masked(grid, x)
    n = len(x)
    live = np.ones(n, bool) if live is None else live
    eq = (m[1:] == m[:-1]) & (live[1:] & live[:-1])[:, None, None]  # [n-1, L, 8]
    other = np.zeros(n - 1, bool) if key_extra is None else key_extra[1:] != key_extra[:-1]
    lane = np.arange(1, n) % width
    inside = eq & (lane != 0)[:, None, None] & ~other[:, None, None]
    longest, run = 1, np.ones(m.shape[1:], np.int64)
    for i in range(n - 1):
        run = np.where(inside[i], run + 1, 1)
        longest = max(longest, int(run.max()))
    groups = -(-n // width)
    norun = sum(int((~inside[g * width: (g + 1) * width - 1].any(0)).sum()) for g in range(groups) if (g + 1) * width <= n)
    return dict(merged=int(inside.sum()), across=int((eq & (lane == 0)[:, None, None]).sum()), longest=longest,
                groups_without_run=int(norun), other_grid=int((eq & other[:, None, None]).sum()))


def census_slices(grid: Grid, x, plan: dict, row_offset=None) -> dict:
    """the partition: x-pairs whose floor and ceil corner lie in different slices (two records), slices no record reaches (the
    cnt == 0 fill), slices in all"""
    _, m = _masked(grid, x)
    keep = np.ones(len(x), bool) if row_offset is None else np.asarray(row_offset) >= 0
    ts = plan["log2TS"]
    straddle = sum(int((((m[keep][..., f] ^ m[keep][..., c]) >> ts) != 0).sum()) for f, c in zip(PAIR_F, PAIR_C))
    col = (np.arange(grid.L)[None, :, None] * (grid.T >> ts)) + (m >> ts)
    if row_offset is not None:
        col = col + (np.maximum(np.asarray(row_offset, np.int64), 0) // grid.rows * (grid.L * (grid.T >> ts)))[:, None, None]
    hit = np.unique(col[keep])
    total = grid.L * plan["nb"]
    return dict(straddle=straddle, empty=total - len(hit), slices=total)


def coherent_chunk(r: Rays, first: int, count: int) -> int:
    """coherent_rays_of (csrc/encode_bwd_binned.hip), restated: rays of a chunk walked sample-index-major, 0: ray-major"""
    S = r.starts.shape[1]
    if S < 16 or S > CHUNK // 16 or CHUNK % S or count < CHUNK:
        return 0
    nr = CHUNK // S
    r0 = first // S
    o, d = r.origins.astype(f32), r.directions.astype(f32)
    tol = f32(1e-4) * (f32(1) + np.abs(o[r0]).sum(dtype=f32))
    same_o = all(np.abs(o[k] - o[r0]).sum(dtype=f32) <= tol for k in (r0 + 1, r0 + nr - 1))
    c1, c2 = (d[r0] * d[r0 + 1]).sum(dtype=f32), (d[r0] * d[r0 + nr - 1]).sum(dtype=f32)
    return nr if same_o and c1 > f32(0.9999) and c2 > f32(0.99) else 0


def live_per_chunk(go) -> list:
    """live samples (a gradient row with any non-zero) per 4096-sample chunk"""
    live = (np.asarray(go) != 0).any(1)
    return [int(live[a:a + CHUNK].sum()) for a in range(0, len(live), CHUNK)]
