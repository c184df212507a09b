"""Cases, references and bounds for the fused render kernel (csrc/render.hip: nrhip::render_kernel, every row of
csrc/render_variants.h whose source is Static, EvalTable or Overrides): tests/test_render_exact_refs_host.py on the CPU,
tests/test_gpu_render_exact.py on the GPU.  One right answer per sample and per ray, where the older tests hold whole
tensors to a norm.

THE LATTICE FAMILY: every operand is an integer, every output has ONE right answer, bit for bit.
  grid       every scaling is a power of two >= 64 (GRIDS), T = 2^11, static_scale = 16, pixel_area = 0 (std = 0, the rescale
             weight is rcp(max(0, 1)) = 1)
  positions  origins are integers, directions a signed unit axis or 0, every interval [c - 1, c + 1] (or [c - 1/2, c + 1/2])
             has an integer midpoint c, and |o + d c|_inf <= 15: the contracted coordinate (q / 16 + 2) / 4 = (q + 32) / 64 is a
             multiple of 1 / 64 in (1/4, 3/4), floor == ceil at every level, all eight corners are ONE table row and the blend
             fma(f, 0, f * 1) returns it.  Bins need not be monotone along a ray where starts and ends are separate tensors:
             a ray revisits its line's points in any order, which is how S reaches 129 on a line of at most 30 points
  network    the table holds integers in [-3, 3] (exact in fp16 storage), all weights and biases are small integers, the SH
             columns of fw0 are zero (the per-ray bias row is fb0 + 0 * sh = fb0), row 0 of gw1 is 256 x a row of -1 / 0 / 1 and
             its bias is 128: the raw head value is 256 k + 128, |value| >= 128
`assert_exact_operands` demands S = sum |a||b| + |bias| < 2^24 for every output of every layer: every partial sum of any
subset of the terms, in any order and grouping, is then an integer below 2^24 and no fp32 operation has anything to round
(tests/mlp_refs.py has the argument in full).  Under each product form (render_variants.h: Prod):
  F32        v_mfma_f32_16x16x4_f32 onto the bias: fp32 products and sums of integers, exact by the argument above.  Row 0 of
             gw1 (the sdf) is an fmaf chain and two cross-lane adds on the vector ALU in EVERY form: the same argument, with
             the row's 256 inside S
  F16Pairs   (mfma_layer_pairs) the tile runs in units of 2^6 and the weights are staged x 2^7.  A layer takes the pair
             products for a tile only if every input of its 16 samples is below 65000 / 64 = 1015.6 in magnitude: 64 n with
             |n| <= 1015 has at most 10 significant bits and is below fp16's 65504, so hi = fp16(64 n) is exact and lo = 0;
             128 w with |w| <= 3 is exact in fp16 and its lo is 0.  The products are multiples of 2^13 that v_mfma_f32_16x16x32_f16
             adds onto 2^13 x bias in fp32: all partial sums are 2^13 x (an integer below 2^24), exact; the 2^-7 afterwards and
             the 2^-6 at the three exits are powers of two.  A layer whose inputs do not fit takes v_mfma_f32_16x16x4_f32 on
             the same scaled operands: exact for the same reason.  `pair_layers` says from the reference activations which
             (tile, layer) takes which; the family holds both kinds (test_lattice_family_holds_pair_and_fallback_tiles)
  Bf16Split  (mfma_layer_split) x = h + m + l by truncation to 8 significant bits each, six of the nine cross terms are
             kept (h.h, h.m, m.h, m.m, h.l, l.h).  An integer |x| < 2^16 has l = 0 and a weight |w| < 2^8 has m = l = 0: the
             kept terms h_w.h_x + h_w.m_x are the whole product, each exact, summed in fp32.  This form is NOT exact for
             arbitrary integers below 2^24, so its cases are restricted: `assert_exact_operands(split=True)` demands
             |activation| < 2^16 and |weight| < 2^8 (the lattice networks have |w| <= 3 and activations below 2^16 at H = 64)
SELECTOR COMPOSITING.  With |raw| >= 128 and beta >= 1 the head saturates exactly: __expf(sdf beta) overflows to inf or is
below 2^-126 (1 + it == 1), alpha = rcp(inf) = 0 or rcp(1) = 1; the density head gives expf(raw) = inf or 0, sigma delta = inf
or 0 (delta > 0 always), 1 - exp(-inf) = 1.  The transmittance is a product of 0s and 1s (a sum of 0s and infs), every weight is
exactly 0 or 1 and the one 1 sits on the FIRST hit: the ray's features are that sample's integer feature (fw2 . h2 + fb2 x 1 +
embedding: integers again), accumulation 1, depth the hit's midpoint.  Dense samples: the last sample's depth is dropped
and a ray without a hit gets the last sample's feature through the sky residual 1 - 0, accumulation 0.  Packed samples: the
last sample counts and a ray without a hit, or without samples, gives zeros.  `ray_lists` places the first hit at prescribed
indices from the reference's own hit / miss classification of the line's points.

THE GRADED FAMILY keeps positions and the integer network but row 0 of gw1 is scaled by a power of two (GRADED_ROW0, 2^-3
under the SDF head: the raw value is a multiple of 1/8, still exact) and beta is a power of two with beta_min = 0, so that x = sdf beta is exact and only
__expf, rcp, the transmittance scan and the weighted sums round.  Samples are kept on rays where every |x| <= 4 (density
head: |raw| <= 4): alpha in [0.018, 0.98].  `composite_model` is float64 and returns a bound with every output (U = 2^-24 per
correctly rounded fp32 operation, E = 2^-23 per v_exp_f32 / v_rcp_f32, 2 E per expf as in tests/proposal_refs.py):
  alpha      e = __expf(x) = v_exp_f32(x log2e): the product rounds and log2e is an fp32 constant, 2 U |x| log2e on the exponent,
             ln 2 of that on e, + E:  rel(e) = E + 2 U |x|.  1 + e: U.  rcp: E.        rel(alpha) = (1 - alpha) rel(e) + U + E
  1 - alpha  abs alpha rel(alpha) + U (1 - alpha)
  T_i        a product of i factors formed by i - 1 multiplications inside the 16-lane scans, one per tile for the carry and
             one for carry x excl: rel(T_i) = sum_{j<i} rel(1 - alpha_j) + (i + i // 16 + 1) U;  w = T alpha: + rel(alpha) + U
  density    sigma = expf(raw): 2 E; sigma delta: U; the running sum of i terms: (i + i // 16 + 1) U of the sum of |terms| + the
             terms' own errors; T = expf(-sum): the sum's absolute error + 2 E; 1 - expf(-sd): e^-sd (abs(sd) + 2 E) + U
  weights    + 2^-126 each: a weight below fp32's normal range is flushed or loses bits
  sums       the per-ray outputs are sums  sum_i w_i v_i  of exact integers v (midpoints; h2 and the embedding, the deferred
             last layer fw2 applied once per ray): |error| <= sum_i dw_i A_i + gamma_n sum_i w_i A_i with A the sum of |terms|
             (A_ic = sum_k |fw2_ck| |h2_ik| + |e_ic| + |fb2_c|), n the length of the longest chain of roundings: tiles of the
             ray + H + 6 for the features (per-lane fma chain over the tiles, the H-term product, the embedding add, four
             row-sum steps, the bias fma), 2 x tiles + 4 for depth (product and add round separately), tiles + 4 for the
             accumulation.  The sky sample's weight w_{S-1} + (1 - acc) carries acc's own error and two more roundings.
No bound uses a kernel's output.  Pair products change nothing here: the per-sample activations are exact integers under
them as under fp32 (above), and what rounds -- head, scan, sums -- is the same code in both forms.

THE INTERPOLATING FAMILY: real trilinear blends.  Positions come from tests/proposal_refs.py's exact_case (world coordinates
multiples of 1/32 below static_scale, both contraction faces, pinned coordinates) on ladders that start at 16
(INTERP_GRIDS): the offset at scaling 2^k is a multiple of 2^(k-11), at most 7 bits at the coarsest level, and with table
integers in [-3, 3] the lerp tree's three fma stages hold 7, 14 and 21 fraction bits plus 2 integer bits -- within fp32's 24,
so the float64 lerp is the fp32 one and the saved `enc` rows have one right answer.  Behind the encoding the network's
inputs are no longer integers and every layer rounds: `interp_ref` carries a forward interval bound through |W|,
  |z^ - z| <= |W| dx + gamma_(K + 2) (|W| (|x| + dx) + |b|)     (K inputs accumulated onto the bias; ReLU is 1-Lipschitz)
starting from dx = 0 at the encoding; K + 3 for the sdf row (fmaf chain, two cross-lane adds, the bias).  Pair products add
2^-22 |W||x| (x = fp16 hi + fp16 lo keeps 22 bits) + 2^-30 |W| (the lo half below fp16's normal range, in tile units of 2^6).
`interp_sh_case` puts every sample AT its ray's origin (intervals [-c, c]: t = 0 exactly) so that directions from synth.rays
leave the positions dyadic; with nonzero SH columns in fw0 the SH values (x = (d + 1) / 2 rounds once; constants are fp32;
at most five separately rounded operations on a cubic) are held to 10 U x the polynomial with every term taken absolute,
and that bound enters feature layer 0 with the other 32 inputs.

DEFECTS.  `sample_ref` and `composite_model` take a `defect`: one of DEFECTS planted into an otherwise right evaluation (two
in the samples: a level read for another, two weights of one unit exchanged; three in the compositing);
tests/test_render_exact_refs_host.py shows that each passes rel_l2 < 1e-4 (the older tests' check) and fails the comparison
made here."""
import functools
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import neurad_oracle as O
import proposal_refs as P
import synth
from host_gate import variant_rows
from mlp_refs import imatmul

U = 2.0 ** -24
E = 2.0 ** -23
LIMIT = 2 ** 24
LOG2_T = 11
STATIC_SCALE = 16.0
QMAX = 15  # |world coordinate| of every sample
PAIR_FIT = 65000.0 / 64.0  # mfma_layer_pairs: a layer's inputs below this take the pair products
# (L, F) -> (min_res, max_res): every scaling an exact power of two >= 64 (test_grids_are_powers_of_two)
GRIDS = {(8, 4): (64, 8192), (16, 2): (64, 1 << 21), (4, 8): (64, 4096), (4, 2): (64, 4096), (1, 4): (64, 64),
         (8, 2): (64, 8192), (4, 4): (64, 512)}
# the interpolating family's ladders: powers of two from 16 (offsets of at most 7 bits at the coarsest level)
INTERP_GRIDS = {(8, 4): (16, 2048), (16, 2): (16, 1 << 19), (4, 8): (16, 1024), (4, 2): (16, 1024), (1, 4): (16, 16),
                (8, 2): (16, 2048), (4, 4): (16, 1024)}
SOURCES = ("Static", "EvalTable", "Overrides")  # Actors / PackedActors rows: tests/actor_refs.py's business
DEFECTS = ("level_swap", "sky_on_s_minus_2", "last_depth", "weight_column", "dead_lane_alpha")
GRADED_ROW0 = {True: 2.0 ** -3, False: 2.0 ** -5}  # graded family, by use_sdf: scale of gw1 row 0 and its bias
TINY = 2.0 ** -126  # below it fp32 flushes or loses bits: an absolute term on every weight
CAP = 4.0  # graded family: |x| of every sample of a kept ray


def rows(outputs=("PerSample", "Composite"), sources=SOURCES, products=("F32", "F16Pairs", "Bf16Split")):
    """the rows of NRHIP_RENDER_VARIANTS in scope, as (L, F, H, output, source, products)"""
    return [r for r in variant_rows() if r[3] in outputs and r[4] in sources and r[5] in products]


# ---- networks ----------------------------------------------------------------------------------------------------------------
def _sparse(rng, shape, values, density):
    return (rng.choice(values, shape) * (rng.random(shape) < density)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def network(L, F, H, use_sdf=True, graded=False, sh=False, seed=0, interp=False, lg=LOG2_T):
    """O.FieldParams of the integer network on the (L, F) grid.  graded: row 0 of gw1 x GRADED_ROW0 in place of 256, beta a power of
    two, beta_min 0.  interp: the interpolating family's ladder (INTERP_GRIDS), row 0 of gw1 a row of -1 / 0 / 1; sh: nonzero
    (integer) SH columns in fw0 -- that family's second case only.  lg: log2 of the table size where it is not 2^11 (the
    eval-table case with a shadow level; call network.__wrapped__ for it: such a table is not worth keeping)"""
    rng = np.random.default_rng([seed, L, F, H])
    mn, mx = (INTERP_GRIDS if interp else GRIDS)[(L, F)]
    LF = L * F
    table = (rng.integers(-3, 4, (L << lg, F)) if lg == LOG2_T else rng.integers(-3, 4, (L << lg, F), np.int8)).astype(np.float32)
    grid = O.GridParams(table, L, mn, mx, lg)
    ints = lambda lo, hi, n: rng.integers(lo, hi + 1, n).astype(np.float32)  # noqa: E731
    gw0 = _sparse(rng, (H, LF), [-1.0, 1.0], min(1.0, 16.0 / LF))
    gw1 = _sparse(rng, (33, H), [-2.0, -1.0, 1.0, 2.0], 0.5)
    gw1[0] = _sparse(rng, (H,), [-1.0, 1.0], 0.5)
    gb1 = ints(-2, 2, 33)
    fw0 = np.zeros((H, 48), np.float32)
    fw0[:, :32] = _sparse(rng, (H, 32), [-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], 0.75)
    if sh:
        fw0[:, 32:] = ints(-2, 2, (H, 16))
    fw1 = _sparse(rng, (H, H), [-1.0, 1.0], 0.25)
    fw2 = _sparse(rng, (32, H), [-1.0, 1.0], 0.25)
    gw0[0], fw0[1], fw1[2] = 0.0, 0.0, 0.0  # units with a zero row ...
    gb0, fb0, fb1, fb2 = ints(-2, 2, H), ints(-2, 2, H), ints(-2, 2, H), ints(-3, 3, 32)
    gb0[0], fb0[1], fb1[2] = 0.0, 0.0, 0.0  # ... and a zero bias: z == 0 exactly, ReLU must mask it
    # row 0 of gw1, centred: the bias takes the median of w0 . hg over lattice points away, so that hits and misses (graded:
    # both signs of the raw value) are about equally frequent
    if interp:
        return O.FieldParams(grid, STATIC_SCALE, [gw0, gw1], [gb0, gb1], [fw0, fw1, fw2], [fb0, fb1, fb2], beta=2.0 ** -2,
                             beta_min=0.0, use_sdf=use_sdf)
    q = rng.integers(-QMAX, QMAX + 1, (2048, 3))
    enc = table[lattice_rows(grid, q)].reshape(len(q), -1)
    k0 = np.median(np.maximum(enc @ gw0.T + gb0, 0) @ gw1[0])
    gb1[0] = -np.floor(k0)
    if graded:
        gw1[0] *= GRADED_ROW0[use_sdf]
        gb1[0] *= GRADED_ROW0[use_sdf]
        beta, beta_min = (2.0 ** -2 if use_sdf else 1.0), 0.0
    else:
        gw1[0] *= 256.0
        gb1[0] = gb1[0] * 256.0 + 128.0
        beta, beta_min = 1.0, 1e-4
    return O.FieldParams(grid, STATIC_SCALE, [gw0, gw1], [gb0, gb1], [fw0, fw1, fw2], [fb0, fb1, fb2], beta=beta,
                         beta_min=beta_min, use_sdf=use_sdf)


def row0_scale(p):
    """the power of two that makes row 0 of gw1 and its bias integers again"""
    m = float(np.abs(p.geo_w[1][0]).max())
    return 1.0 if m == 0 else 2.0 ** min(0, int(np.floor(np.log2(m))))


# ---- the per-sample reference ------------------------------------------------------------------------------------------------
def lattice_rows(grid, q):
    """q [N, 3] integer world coordinates -> [N, L] the ONE table row each level of O.GridParams `grid` reads (level offset
    included)"""
    q = np.asarray(q, np.int64)
    assert (np.abs(q) <= QMAX).all()
    scal = grid.scalings.astype(np.int64)
    n = (q[:, None, :] + 32) * (scal[None, :, None] // 64)  # (q + 32) / 64 * scaling: an integer
    lo = (np.arange(grid.num_levels, dtype=np.int64) * grid.table_size)[None, :]
    return O.hash_indices(n.astype(np.int32), grid.table_size, lo)


@dataclass
class Samples:
    """int64 activations of N samples (sdf: float64, row0_scale x an integer).  hf = [hf0 | hf1]"""
    enc: np.ndarray  # [N, L * F]
    hg: np.ndarray  # [N, H]
    emb: np.ndarray  # [N, 32] = xf[:, :32]
    hf: np.ndarray  # [N, 2 H]
    sdf: np.ndarray  # [N]
    feature: np.ndarray  # [N, 32]
    smax: float  # the largest sum |a||b| + |bias| of any output of any layer
    amax: int  # the largest |activation| that enters a matrix product


def _int(a):
    r = np.asarray(a, np.float64)
    out = r.astype(np.int64)
    assert (out == r).all()
    return out


def mlp_ref(p, enc, defect=None):
    """the five layers on integer encoding rows enc [N, L * F], exactly.  defect ("weight_column", n, a, b): the weights of
    inputs a and b of unit n of fw1 exchanged (a K-axis permutation inside one weight fragment)"""
    s0 = row0_scale(p)
    gw0, gw1 = _int(p.geo_w[0]), _int(np.concatenate([p.geo_w[1][:1] / s0, p.geo_w[1][1:]]))
    gb0, gb1 = _int(p.geo_b[0]), _int(np.concatenate([p.geo_b[1][:1] / s0, p.geo_b[1][1:]]))
    fw0, fw1, fw2 = _int(p.feat_w[0][:, :32]), _int(p.feat_w[1]), _int(p.feat_w[2])
    fb0, fb1, fb2 = (_int(b) for b in p.feat_b)
    if defect is not None and defect[0] == "weight_column":
        _, n, a, b = defect
        fw1 = fw1.copy()
        fw1[n, [a, b]] = fw1[n, [b, a]]
    enc = np.asarray(enc, np.int64)
    smax, amax = 0.0, int(np.abs(enc).max(initial=0))

    def layer(x, w, b):
        nonlocal smax, amax
        smax = max(smax, float((imatmul(np.abs(x), np.abs(w).T) + np.abs(b)).max(initial=0)))
        amax = max(amax, int(np.abs(x).max(initial=0)))
        return imatmul(x, w.T) + b

    hg = np.maximum(layer(enc, gw0, gb0), 0)
    geo = layer(hg, gw1, gb1)
    emb = geo[:, 1:]
    hf0 = np.maximum(layer(emb, fw0, fb0), 0)
    hf1 = np.maximum(layer(hf0, fw1, fb1), 0)
    feature = layer(hf1, fw2, fb2) + emb
    smax = max(smax, float((imatmul(np.abs(hf1), np.abs(fw2).T) + np.abs(fb2) + np.abs(emb)).max(initial=0)))
    return Samples(enc, hg, emb, np.concatenate([hf0, hf1], 1), geo[:, 0].astype(np.float64) * s0, feature, smax, amax)


def sample_ref(p, q, ovr_row=None, ovr_rows=None, defect=None):
    """the reference of samples at integer world coordinates q [N, 3]; ovr_row [N] (-1 or a row of ovr_rows [P, L * F]): the
    samples that take their encoding row from the caller.  Distinct positions are evaluated once.
    defect ("level_swap", i): sample i reads level 1's row for level 0 and level 0's for level 1; ("weight_column", ...): see
    mlp_ref"""
    q = np.asarray(q, np.int64)
    uq, inv = np.unique(q, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    enc_u = _int(p.grid.table[lattice_rows(p.grid, uq)]).reshape(len(uq), -1)
    if ovr_row is None and defect is None:
        u = mlp_ref(p, enc_u)
        return Samples(u.enc[inv], u.hg[inv], u.emb[inv], u.hf[inv], u.sdf[inv], u.feature[inv], u.smax, u.amax)
    enc = enc_u[inv]
    if defect is not None and defect[0] == "level_swap":
        F, i = p.grid.n_feat, defect[1]
        enc[i, :2 * F] = np.concatenate([enc[i, F:2 * F], enc[i, :F]])
    if ovr_row is not None:
        hit = np.asarray(ovr_row) >= 0
        enc[hit] = _int(ovr_rows)[np.asarray(ovr_row)[hit]]
    return mlp_ref(p, enc, defect)


def assert_exact_operands(ref, split=False):
    """a condition on the operands: every sum of |products| below 2^24; split: the 3-way bf16 form's restriction as well.
    -> the largest sum"""
    assert ref.smax < LIMIT, ref.smax
    if split:
        assert ref.amax < 2 ** 16, ref.amax
    return ref.smax


def is_hit(p, sdf):
    """the saturated head of the lattice family: alpha == 1 (density == inf)"""
    assert (np.abs(sdf) * (abs(p.beta) + p.beta_min if p.use_sdf else 1.0) >= 100).all()
    return sdf < 0 if p.use_sdf else sdf > 0


@functools.lru_cache(maxsize=None)
def hit_lattice(L, F, H, use_sdf):
    """[31, 31, 31] bool: the classification of every lattice point by the lattice network's own reference"""
    return classify_lattice(network(L, F, H, use_sdf))


def classify_lattice(p):
    ax = np.arange(-QMAX, QMAX + 1)
    q = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    enc = _int(p.grid.table[lattice_rows(p.grid, q)]).reshape(len(q), -1)
    s0 = row0_scale(p)
    hg = np.maximum(imatmul(enc, _int(p.geo_w[0]).T) + _int(p.geo_b[0]), 0)
    sdf = (imatmul(hg, _int(p.geo_w[1][:1] / s0).T)[:, 0] + _int(p.geo_b[1][:1] / s0)[0]) * s0
    return is_hit(p, sdf).reshape(31, 31, 31)


# ---- rays --------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """rays on lattice lines.  t: the integer midpoints, ray after ray; seg [R + 1]: ray r owns t[seg[r]:seg[r + 1]].
    half: intervals [c - half, c + half]"""
    o: np.ndarray  # [R, 3] fp32 integers
    d: np.ndarray  # [R, 3] a signed unit axis, or 0
    t: np.ndarray  # [M] int64
    seg: np.ndarray  # [R + 1] int64
    want: List[Optional[int]]  # per ray: the prescribed first hit (None: no hit), -1: left to chance
    half: float = 1.0

    @property
    def R(self):
        return self.o.shape[0]

    @property
    def counts(self):
        return np.diff(self.seg)

    @property
    def ray_of(self):
        return np.repeat(np.arange(self.R), self.counts)

    @property
    def q(self):
        r = self.ray_of
        return (self.o[r].astype(np.int64) + self.d[r].astype(np.int64) * self.t[:, None])

    @property
    def area(self):
        return np.zeros(self.R, np.float32)

    def dense(self):
        """-> starts, ends [R, S] fp32 (every ray has S samples)"""
        S = int(self.counts[0])
        assert (self.counts == S).all()
        t = self.t.reshape(self.R, S).astype(np.float32)
        return t - np.float32(self.half), t + np.float32(self.half)

    def packed(self):
        """-> t_starts, t_ends [M] fp32, segments [R + 1] int64"""
        t = self.t.astype(np.float32)
        return t - np.float32(self.half), t + np.float32(self.half), self.seg.astype(np.int64)

    def edges(self):
        """monotone rays (edge_case) -> [R, S + 1] fp32: starts / ends are views of it"""
        S = int(self.counts[0])
        t = self.t.reshape(self.R, S).astype(np.float32)
        assert (np.diff(t, axis=1) == 2 * self.half).all()
        return np.concatenate([t - np.float32(self.half), t[:, -1:] + np.float32(self.half)], 1)


def prescribed(n):
    """the first-hit indices a ray of n samples is asked for: 0, 15, 16, 17, 63, 64, n - 2, n - 1 where they exist, and none"""
    return sorted({i for i in (0, 15, 16, 17, 63, 64, n - 2, n - 1) if 0 <= i < n}) + [None]


def ray_lists(hits, counts, seed, still_every=2):
    """rays whose first hit sits where `prescribed` says, the k-th ray of n samples taking entry k of n's list (cyclically): a ray along an
    axis through the lattice draws the samples before its first hit from the line's misses, the hit from the line's hits
    and the rest from both.  Of the rays asked for a first hit at 0 or for none, every `still_every`-th round stands still
    (d = 0: ONE position, a hit or a miss).  hits: hit_lattice(...)"""
    rng = np.random.default_rng([seed, len(counts), int(np.sum(counts))])
    o, d, ts, want, nth = [], [], [], [], {}
    for n in (int(c) for c in counts):
        opts = prescribed(n) if n else [None]
        k = nth[n] = nth.get(n, -1) + 1  # the k-th ray of n samples takes entry k of its list
        w = opts[k % len(opts)]
        still = bool(still_every) and w in (0, None) and (k // len(opts)) % still_every == 0
        for _ in range(1000):
            oo, dd = rng.integers(-QMAX, QMAX + 1, 3), np.zeros(3, np.int64)
            if still:
                line_t = np.arange(1, 31)
                cls = np.full(30, hits[tuple(oo + QMAX)])
            else:
                k, sgn = int(rng.integers(0, 3)), int(rng.choice([-1, 1]))
                dd[k] = sgn
                oo[k] = -sgn * int(rng.integers(8, QMAX + 1))
                line_t = np.arange(1, QMAX + abs(int(oo[k])) + 1)
                cls = hits[tuple((oo[None, :] + dd[None, :] * line_t[:, None] + QMAX).T)]
            miss_t, hit_t = line_t[~cls], line_t[cls]
            if n == 0 or not (((w is None or w > 0) and len(miss_t) == 0) or (w is not None and len(hit_t) == 0)):
                break
        else:
            raise AssertionError("no line realises the prescription")
        if n and w is None:
            ts.append(rng.choice(miss_t, n))
        elif n:
            ts.append(np.concatenate([rng.choice(miss_t, w) if w else np.zeros(0, np.int64), rng.choice(hit_t, 1),
                                      rng.choice(line_t, n - w - 1)]))
        o.append(oo), d.append(dd), want.append(w)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t = np.concatenate(ts).astype(np.int64) if ts else np.zeros(0, np.int64)
    return Case(np.array(o, np.float32).reshape(-1, 3), np.array(d, np.float32).reshape(-1, 3), t, seg, want)


def dense_case(L, F, H, use_sdf, R, S, seed=0):
    return ray_lists(hit_lattice(L, F, H, use_sdf), [S] * R, seed)


def packed_case(L, F, H, use_sdf, counts, seed=0):
    return ray_lists(hit_lattice(L, F, H, use_sdf), list(counts), seed)


# packed segment layouts: every count of the issue, empty rays first, last and two in a row, M = 1
PACKED_COUNTS = {"mixed": (0, 0, 17, 64, 1, 65, 0, 0, 16, 15, 0), "one_sample": (1,), "one_between_empty": (0, 1, 0),
                 "tail_empty": (65, 17, 16, 0, 0), "many": (17, 1, 0, 65, 16, 15, 64, 0, 0) * 9}


def edge_case(R, S, seed=0, half=0.5):
    """monotone rays for starts / ends as views of one edge tensor: consecutive integer midpoints (S <= 30) on moving rays,
    every fourth ray standing still; hits fall where the line has them"""
    assert S <= 30
    rng = np.random.default_rng([seed, R, S, 7])
    o = rng.integers(-QMAX, QMAX + 1, (R, 3))
    d = np.zeros((R, 3), np.int64)
    t0 = np.ones(R, np.int64)
    for r in range(R):
        if r % 4 == 3:
            t0[r] = rng.integers(1, 5)
            continue
        k, sgn = int(rng.integers(0, 3)), int(rng.choice([-1, 1]))
        d[r, k] = sgn
        o[r, k] = -sgn * QMAX
        t0[r] = rng.integers(1, 30 - S + 2)  # coordinates -15 + t, t in [t0, t0 + S - 1] <= 30
    t = t0[:, None] + np.arange(S)[None, :]
    seg = (np.arange(R + 1) * S).astype(np.int64)
    return Case(o.astype(np.float32), d.astype(np.float32), t.reshape(-1), seg, [-1] * R, half)


def first_hits(case, hit):
    """hit [M] bool -> per ray the index of its first hit, or -1"""
    out = np.full(case.R, -1, np.int64)
    for r in range(case.R):
        h = np.flatnonzero(hit[case.seg[r]:case.seg[r + 1]])
        if len(h):
            out[r] = h[0]
    return out


# ---- compositing -------------------------------------------------------------------------------------------------------------
@dataclass
class Rays:
    features: np.ndarray  # [R, 32]
    depth: np.ndarray  # [R, 1]
    accumulation: np.ndarray  # [R, 1]
    weights: np.ndarray  # [M]


def selector_ref(p, case, ref, packed):
    """the lattice family's composited outputs: one sample's integers per ray (see SELECTOR COMPOSITING above)"""
    first = first_hits(case, is_hit(p, ref.sdf))
    R, M = case.R, len(case.t)
    feats, depth, acc, w = np.zeros((R, 32)), np.zeros((R, 1)), np.zeros((R, 1)), np.zeros(M)
    for r in range(R):
        b, n = int(case.seg[r]), int(case.counts[r])
        if n == 0:
            continue
        if first[r] >= 0:
            i = b + first[r]
            feats[r], acc[r], w[i] = ref.feature[i], 1.0, 1.0
            if packed or first[r] < n - 1:
                depth[r] = case.t[i]
        elif not packed:
            feats[r] = ref.feature[b + n - 1]
    return Rays(feats, depth, acc, w)


@dataclass
class Graded:
    alpha: np.ndarray  # [M] (density head: the density)
    alpha_bound: np.ndarray
    rays: Rays
    bound: Rays
    keep: np.ndarray  # [R] bool: every |x| <= CAP


def _gamma(n):
    return n * U / (1 - n * U)


def composite_model(p, case, ref, packed, defect=None, bounds=True):
    """float64 compositing of the per-sample reference `ref` with generic alphas, and the bound of every output (module
    docstring).  defect: "sky_on_s_minus_2" (the residual 1 - acc on sample S - 2), "last_depth" (dense: the last sample's depth
    counted), "dead_lane_alpha" (the lanes behind a ragged ray's end hold its last sample: their alpha enters the
    accumulation, with the transmittance running on)"""
    R, M = case.R, len(case.t)
    delta = 2.0 * case.half
    x = ref.sdf * (abs(p.beta) + p.beta_min) if p.use_sdf else ref.sdf
    if p.use_sdf:
        with np.errstate(over="ignore"):
            e = np.exp(x)
        a = 1.0 / (1.0 + e)
        rel_a = (1 - a) * (E + 2 * U * np.abs(x)) + U + E
        head, head_bound = a, a * rel_a
    else:
        sig = np.exp(x)
        head, head_bound = sig, sig * 2 * E
    A = imatmul(np.abs(ref.hf[:, ref.hf.shape[1] // 2:]), np.abs(_int(p.feat_w[2])).T) + np.abs(ref.emb) \
        + np.abs(_int(p.feat_b[2]))[None, :]
    H = ref.hg.shape[1]
    out = Rays(np.zeros((R, 32)), np.zeros((R, 1)), np.zeros((R, 1)), np.zeros(M))
    bnd = Rays(np.zeros((R, 32)), np.zeros((R, 1)), np.zeros((R, 1)), np.zeros(M))
    keep = np.ones(R, bool)
    for r in range(R):
        b, n = int(case.seg[r]), int(case.counts[r])
        if n == 0:
            continue
        sl = slice(b, b + n)
        i = np.arange(n)
        steps = (i + i // 16 + 1)
        keep[r] = bool((np.abs(x[sl]) <= CAP).all())
        if p.use_sdf:
            al, om = a[sl], 1 - a[sl]
            rel_om = al * rel_a[sl] / om + U
            T = np.concatenate([[1.0], np.cumprod(om)[:-1]])
            rel_T = np.concatenate([[0.0], np.cumsum(rel_om)[:-1]]) + steps * U
            w = T * al
            dw = w * (rel_T + rel_a[sl] + U) + TINY
        else:
            sd = sig[sl] * delta
            d_sd = sd * (2 * E + U)
            cs = np.concatenate([[0.0], np.cumsum(sd)[:-1]])
            d_cs = np.concatenate([[0.0], np.cumsum(d_sd)[:-1]]) + steps * U * cs
            T = np.exp(-cs)
            al = 1 - np.exp(-sd)
            d_al = np.exp(-sd) * (d_sd + 2 * E) + U * al
            w = T * al
            dw = w * (d_cs + 2 * E + U) + T * d_al + TINY
        tiles = (n + 15) // 16
        acc_w = w.sum()
        if defect == "dead_lane_alpha" and n % 16:
            dead = 16 - n % 16
            last_a = al[-1]
            acc_w += (T[-1] * (1 - last_a) * last_a * (1 - last_a) ** np.arange(dead)).sum()
        d_acc = dw.sum() + _gamma(tiles + 4) * w.sum()
        wf, dwf = w.copy(), dw.copy()
        if not packed:
            k = n - 2 if (defect == "sky_on_s_minus_2" and n > 1) else n - 1
            wf[k] += 1 - acc_w
            dwf[k] += d_acc + 2 * U * (abs(1 - acc_w) + w[k])
        out.weights[sl], bnd.weights[sl] = w, dw
        out.accumulation[r], bnd.accumulation[r] = acc_w, d_acc
        f = ref.feature[sl].astype(np.float64)
        out.features[r] = wf @ f
        last = n if (packed or defect == "last_depth") else n - 1
        mid = case.t[sl].astype(np.float64)
        out.depth[r] = (w[:last] * mid[:last]).sum()
        if bounds:
            Ar = A[sl].astype(np.float64)
            bnd.features[r] = dwf @ Ar + _gamma(tiles + H + 6) * (wf @ Ar) \
                + np.abs(_int(p.feat_b[2])) * ((2 * U) if not packed else (d_acc + U * acc_w))
            bnd.depth[r] = (dw[:last] * mid[:last]).sum() + _gamma(2 * tiles + 4) * (w[:last] * mid[:last]).sum()
    return Graded(head, head_bound, out, bnd, keep)


def oracle_inputs(case):
    """(origins, directions, pixel_area, starts, ends) of a dense case for oracle/neurad_oracle.py"""
    s, e = case.dense()
    return case.o, case.d, case.area, s, e


# ---- overrides ---------------------------------------------------------------------------------------------------------------
def override_case(L, F, case, seed=0):
    """(ovr_row int32 [M], ovr_rows [P, L * F] integers in [-3, 3], ovr_dirs [P, 3] unit vectors): on every third ray the
    samples 5 (a full tile), 50 (the last tile of a 64-sample block) and n - 1 (the ragged tile where n % 16 != 0) take
    their rows from the caller, where the ray's n samples reach them"""
    rng = np.random.default_rng([seed, L, F, len(case.t), case.R])
    ovr = np.full(len(case.t), -1, np.int32)
    picks = sorted({int(case.seg[r]) + s for r in range(0, case.R, 3) for s in (5, 50, int(case.counts[r]) - 1)
                    if 0 <= s < case.counts[r]})
    P = len(picks) + 2  # (two rows nobody uses)
    ovr[picks] = rng.permutation(P)[:len(picks)]
    rows_ = rng.integers(-3, 4, (P, L * F)).astype(np.float32)
    dirs = rng.normal(size=(P, 3))
    return ovr, rows_, (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)


# ---- which (tile, layer) takes the pair products -------------------------------------------------------------------------------
def pair_layers(case, ref):
    """[tiles, 4] bool: does the layer (geo 0, geo 1, feature 0, feature 1) of the 16-sample tile take the fp16-pair
    products -- every input of its samples below PAIR_FIT (mfma_layer_pairs tests each layer's inputs, tile by tile)"""
    H = ref.hg.shape[1]
    ins = [np.abs(ref.enc).max(1), np.abs(ref.hg).max(1), np.abs(ref.emb).max(1), np.abs(ref.hf[:, :H]).max(1)]
    m = np.stack(ins, 1).astype(np.float64)  # [M, 4]
    out = []
    for r in range(case.R):
        b, n = int(case.seg[r]), int(case.counts[r])
        for t0 in range(0, n, 16):
            out.append(m[b + t0:b + min(t0 + 16, n)].max(0) < PAIR_FIT)
    return np.array(out).reshape(-1, 4)


# ---- the interpolating family ---------------------------------------------------------------------------------------------------
@dataclass
class InterpCase:
    o: np.ndarray  # [R, 3]
    d: np.ndarray  # [R, 3]
    starts: np.ndarray  # [R, S]
    ends: np.ndarray  # [R, S]

    @property
    def R(self):
        return self.o.shape[0]

    @property
    def S(self):
        return self.starts.shape[1]

    @property
    def area(self):
        return np.zeros(self.R, np.float32)

    def rays(self):
        return self.o, self.d, self.area, self.starts, self.ends


def interp_case(n, seed=0, shape=None):
    """the positions of proposal_refs.exact_case at n = R * S samples"""
    c = P.exact_case(n, 1, seed, shape)
    return InterpCase(c.o, c.d, np.ascontiguousarray(c.edges[:, :-1]), np.ascontiguousarray(c.edges[:, 1:]))


def interp_sh_case(R, S, seed=0):
    """every sample at its ray's origin (t = 0), directions from synth.rays: dyadic positions under arbitrary directions"""
    c = P.exact_case(R, 1, seed, (R, 1))
    o = np.where((c.regime == P.INSIDE)[:, None], c.o, np.float32(0.25) * np.round(c.o))  # (the faces need d = 0 on an axis)
    o = np.clip(o, -15.0, 15.0).astype(np.float32)
    half = (np.arange(1, S + 1, dtype=np.float32) / np.float32(8))[None, :].repeat(R, 0)
    return InterpCase(o, synth.rays(R, seed + 1)[1].astype(np.float32), -half, half.copy())


def interp_positions(case):
    """float64 contracted positions [N, 3] in [0, 1] (exact: tests/proposal_refs.py: forward_ref)"""
    o, d = case.o.astype(np.float64), case.d.astype(np.float64)
    t0, t1 = case.starts.astype(np.float64), case.ends.astype(np.float64)
    t = t0 + (t1 - t0) / 2
    m = (o[:, None, :] + d[:, None, :] * t[..., None]) / STATIC_SCALE
    mag = np.abs(m).max(-1)
    cm = np.maximum(mag, 1.0)
    m = np.where(~(mag < 1)[..., None], (2 - 1 / cm)[..., None] * (m / cm[..., None]), m)
    return ((m + 2) / 4).reshape(-1, 3)


def sh_ref(d):
    """-> (16 SH values of (d + 1) / 2 in float64 [N, 16], their bound): 10 U x the polynomial with every term absolute"""
    x, y, z = ((d.astype(np.float64)[:, k] + 1) / 2 for k in range(3))
    xx, yy, zz = x * x, y * y, z * z
    k1, k2, k3, k4, k5 = 0.4886025119029199, 1.0925484305920792, 0.9461746957575601, 0.31539156525251999, 0.5462742152960396
    k6, k7, k8, k9, k10 = 0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277
    one = np.ones_like(x)
    val = [0.28209479177387814 * one, k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * zz - k4, k2 * x * z, k5 * (xx - yy),
           k6 * y * (3 * xx - yy), k7 * x * y * z, k8 * y * (5 * zz - 1), k9 * z * (5 * zz - 3), k8 * x * (5 * zz - 1),
           k10 * z * (xx - yy), k6 * x * (xx - 3 * yy)]
    mag = [0.28209479177387814 * one, k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * zz + k4, k2 * x * z, k5 * (xx + yy),
           k6 * y * (3 * xx + yy), k7 * x * y * z, k8 * y * (5 * zz + 1), k9 * z * (5 * zz + 3), k8 * x * (5 * zz + 1),
           k10 * z * (xx + yy), k6 * x * (xx + 3 * yy)]
    return np.stack(val, 1), 10 * U * np.abs(np.stack(mag, 1))


@dataclass
class Interp:
    enc: np.ndarray  # [N, L * F] exact
    val: dict  # name -> float64 value: hg, emb, sh, hf, sdf, feature
    bound: dict  # name -> bound


def _bounded_layer(x, dx, W, b, extra, pairs):
    W, b = W.astype(np.float64), b.astype(np.float64)
    aw = np.abs(W).T
    z = x @ W.T + b
    ax = np.abs(x) @ aw
    dz = dx @ aw + _gamma(W.shape[1] + extra) * (ax + dx @ aw + np.abs(b))
    if pairs:
        dz = dz + 2.0 ** -22 * ax + 2.0 ** -30 * np.abs(W).sum(1)[None, :]
    return z, dz


def interp_ref(p, case, pairs=False):
    """float64 reference of the per-sample kernel on an interpolating case, a bound with every value (module docstring)"""
    pos = interp_positions(case)
    idx, off = O.hashgrid_corner_indices(pos.astype(np.float32), p.grid.scalings, p.grid.table_size)
    assert (pos.astype(np.float32) == pos).all()
    of = off.astype(np.float64)
    cx, cy, cz = of[..., 0], of[..., 1], of[..., 2]
    fx, fy, fz = 1 - cx, 1 - cy, 1 - cz
    w = np.stack([cx * cy * cz, cx * fy * cz, fx * fy * cz, fx * cy * cz, cx * cy * fz, cx * fy * fz, fx * fy * fz, fx * cy * fz], -1)
    enc = (w[..., None] * p.grid.table.astype(np.float64)[idx]).sum(-2).reshape(len(pos), -1)  # [N, L, 8, F] -> [N, L * F]
    H = p.geo_w[0].shape[0]
    z0, d0 = _bounded_layer(enc, np.zeros_like(enc), p.geo_w[0], p.geo_b[0], 2, pairs)
    hg = np.maximum(z0, 0)
    emb, demb = _bounded_layer(hg, d0, p.geo_w[1][1:], p.geo_b[1][1:], 2, pairs)
    sdf, dsdf = _bounded_layer(hg, d0, p.geo_w[1][:1], p.geo_b[1][:1], 3, False)
    sh, dsh = sh_ref(np.repeat(case.d, case.S, 0))
    z1, d1 = _bounded_layer(np.concatenate([emb, sh], 1), np.concatenate([demb, dsh], 1), p.feat_w[0], p.feat_b[0], 2, pairs)
    hf0 = np.maximum(z1, 0)
    z2, d2 = _bounded_layer(hf0, d1, p.feat_w[1], p.feat_b[1], 2, pairs)
    hf1 = np.maximum(z2, 0)
    f, df = _bounded_layer(hf1, d2, p.feat_w[2], p.feat_b[2], 2, False)
    feature, dfeature = f + emb, df + demb + U * (np.abs(f + emb) + df + demb)
    val = {"hg": hg, "emb": emb, "sh": sh, "hf": np.concatenate([hf0, hf1], 1), "sdf": sdf[:, 0], "feature": feature}
    bound = {"hg": d0, "emb": demb, "sh": dsh, "hf": np.concatenate([d1, d2], 1), "sdf": dsdf[:, 0], "feature": dfeature}
    assert H == hg.shape[1]
    return Interp(enc, val, bound)
