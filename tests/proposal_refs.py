"""Cases and float64 references for the stand-alone proposal-density kernels (csrc/hashgrid.hip: proposal_density_fwd /
proposal_levels_lp / proposal_density_from_levels / proposal_density_bwd / proposal_decoder_grad, and the ProposalSrc part of
csrc/encode_bwd_binned.hip).

THE EXACT FAMILY (exact_case).  Every fp32 operation up to the rescaled per-level feature is exact, so `level_features` has
ONE right answer in every kernel and branch, bit for bit:

  grid       scalings are powers of two (GRIDS: min_res 16, max_res chosen per level count), T = 2^11, static_scale = 16
  positions  world coordinates are multiples of 1/32 below static_scale in magnitude (origins multiples of 1/32, |o| <= 5;
             directions in {-1, -1/2, 0, 1/2, 1}; bin edges are sums of steps in {1/8 .. 1/2}, so t is a multiple of 1/16,
             t <= 10).  m / 16 is a multiple of 2^-9, (m + 2) / 4 a multiple of 2^-11 in (1/4, 3/4): at scaling 2^k the
             offset is a multiple of 2^(k-11) -- at most 7 bits at the coarsest level
  features   table values are integers in [-3, 3] (exact in fp16 storage too): the lerp tree's three fmaf stages hold
             7, 14 and 21 fraction bits plus 2 integer bits, within fp32's 24
  rescale    pixel_area = 0: std = exp2(log2(0) / 3) = 0 and rescale_weight = rcp(max(0, 1)) = 1
  regimes    rays r % 8 == 6 run INSIDE the face |m|_inf = 2 * static_scale (cm = 2, k = 1.5; there the other coordinates
             and t are multiples of 1/8, so k * (m / cm) is a multiple of 2^-9 again); rays r % 8 == 7 run inside the face
             |m|_inf = static_scale, the `!(mag < 1)` boundary with k = 1; the rest stay inside.  About one coordinate in
             eight is pinned to a multiple of 4 (direction component 0): its offset is 0 at EVERY level, where floor == ceil.

THE RESCALED FAMILY (rescaled_case): the same positions with pixel_area > 0, so that 2 * scal_l * std crosses 1 between the
coarse and the fine levels.  Only rescale_weight is inexact there; `rtol_rw` bounds it.

The backward references take the exact logit x (float64): gx = g exp(clip(x, -15, 15)) with a NaN kept, d dec_l = sum gx f_l,
d table = index_add of w_k gx dec_l rw."""
from dataclasses import dataclass, replace

import numpy as np

import neurad_oracle as O
from table_grad_refs import log2_slice

U = 2.0 ** -24  # one rounding of a correctly rounded fp32 operation (half an ulp, relative)
E = 2.0 ** -23  # one ulp: v_log_f32, v_exp_f32, v_rcp_f32
LOG2_T = 11
STATIC_SCALE = 16.0
# L -> (min_res, max_res): growth exp((ln max - ln min) / (L - 1)) is 2 or 4, every scaling a power of two
GRIDS = {1: (16, 16), 2: (16, 512), 3: (16, 256), 6: (16, 512), 8: (16, 2048)}
INSIDE, FACE2, FACE1 = 0, 1, 2


def shape_for(n):
    """n = R * S with a small S"""
    S = next(s for s in (7, 5, 4, 3, 2, 1) if n % s == 0)
    return n // S, S


@dataclass
class Case:
    L: int
    o: np.ndarray  # [R, 3]
    d: np.ndarray  # [R, 3]
    area: np.ndarray  # [R]
    edges: np.ndarray  # [R, S + 1]
    table: np.ndarray  # [L * T, 1] fp32, integer values
    dec: np.ndarray  # [1, L] fp32
    regime: np.ndarray  # [R]

    @property
    def R(self):
        return self.o.shape[0]

    @property
    def S(self):
        return self.edges.shape[1] - 1

    @property
    def n(self):
        return self.R * self.S

    @property
    def grid(self):
        mn, mx = GRIDS[self.L]
        return (self.L, 1, LOG2_T, mn, mx)

    @property
    def scalings(self):
        return O.hash_scalings(self.L, *GRIDS[self.L])

    def params(self):
        """the oracle's ProposalParams of this case"""
        mn, mx = GRIDS[self.L]
        return O.ProposalParams(O.GridParams(self.table, self.L, mn, mx, LOG2_T), STATIC_SCALE, self.dec)


def exact_case(n, L=6, seed=0, shape=None):
    """the exact family at n = R * S samples (shape: (R, S) instead of shape_for(n))"""
    R, S = shape or shape_for(n)
    assert R * S == n and S <= 7
    rng = np.random.default_rng([seed, n, L])
    regime = np.where(np.arange(R) % 8 == 6, FACE2, np.where(np.arange(R) % 8 == 7, FACE1, INSIDE))
    o = rng.integers(-160, 161, (R, 3)) / 32.0
    d = rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], (R, 3))
    steps = rng.integers(1, 5, (R, S)) / 8.0
    near = rng.integers(0, 49, (R, 1)) / 8.0
    f2 = regime == FACE2  # everything a multiple of 1/8 there: coordinates, and t through steps and nears of 1/4
    o[f2] = rng.integers(-160, 161, (int(f2.sum()), 3)) / 8.0
    d[f2] = rng.choice([-1.0, 0.0, 1.0], (int(f2.sum()), 3))
    steps[f2] = rng.integers(1, 3, (int(f2.sum()), S)) / 4.0
    near[f2] = rng.integers(0, 25, (int(f2.sum()), 1)) / 4.0
    pin = (rng.random((R, 3)) < 0.125) & (regime == INSIDE)[:, None]  # offsets of 0 at every level
    pin[1::32] = True  # (some rays stand still on such a point: all three offsets 0 at once)
    o[pin] = 4.0 * rng.integers(-1, 2, int(pin.sum()))
    d[pin] = 0.0
    axis, sign = rng.integers(0, 3, R), rng.choice([-1.0, 1.0], R)
    for r in np.flatnonzero(regime != INSIDE):
        o[r, axis[r]] = sign[r] * STATIC_SCALE * (2.0 if regime[r] == FACE2 else 1.0)
        d[r, axis[r]] = 0.0
    edges = np.concatenate([near, near + np.cumsum(steps, 1)], 1)
    table = rng.integers(-3, 4, (L << LOG2_T, 1)).astype(np.float32)
    dec = (rng.permutation(np.r_[-8:0, 1:9])[:L] / 8.0).astype(np.float32)[None, :]  # non-zero, all different
    return Case(L, o.astype(np.float32), d.astype(np.float32), np.zeros(R, np.float32), edges.astype(np.float32), table, dec,
                regime)


def rescaled_case(n, L=6, seed=0):
    """the exact positions with pixel_area in [2^-8, 2^-5]: the contracted std lands between 1 / (2 * 512) and 1 / (2 * 16)
    for most samples, so the coarse levels keep weight 1 and the fine ones are scaled down, inside and on both faces"""
    c = exact_case(n, L, seed)
    rng = np.random.default_rng([seed, n, L, 1])
    return replace(c, area=(2.0 ** rng.uniform(-8.0, -5.0, c.R)).astype(np.float32))


@dataclass
class Forward:
    pos: np.ndarray  # [N, 3] float64, in [0, 1]
    mag: np.ndarray  # [N] |m / static_scale|_inf
    xcb: np.ndarray  # [N] the argument of the first fast_cbrt, area t^2 dist
    std: np.ndarray  # [N] contracted std
    idx: np.ndarray  # [N, L, 8] table rows, level offset included
    w: np.ndarray  # [N, L, 8] corner weights
    interp: np.ndarray  # [N, L] the lerp of the 8 corners
    rw: np.ndarray  # [N, L] rescale weight
    lf: np.ndarray  # [N, L] interp * rw
    x: np.ndarray  # [N] the logit
    ax: np.ndarray  # [N] sum_l |f_l dec_l|


def forward_ref(c):
    """float64 evaluation of the forward from the case's fp32 inputs (NaN table entries propagate like in the kernels:
    a corner of weight 0 still poisons)"""
    o, d, e = c.o.astype(np.float64), c.d.astype(np.float64), c.edges.astype(np.float64)
    t0, t1 = e[:, :-1], e[:, 1:]
    dist = (t1 - t0) / 2
    t = t0 + dist
    m = (o[:, None, :] + d[:, None, :] * t[..., None]) / STATIC_SCALE
    xcb = c.area.astype(np.float64)[:, None] * t * t * dist
    std = np.cbrt(xcb) / STATIC_SCALE
    mag = np.abs(m).max(-1)
    out = ~(mag < 1)
    cm = np.maximum(mag, 1.0)
    m = np.where(out[..., None], (2 - 1 / cm)[..., None] * (m / cm[..., None]), m)
    sc = np.cbrt(2 * cm - 1) / cm
    std = np.where(out, std * sc * sc, std) / 4
    pos = ((m + 2) / 4).reshape(-1, 3)
    scal = c.scalings
    idx, off = O.hashgrid_corner_indices(pos.astype(np.float32), scal, 1 << LOG2_T)
    of = off.astype(np.float64)
    cx, cy, cz = of[..., 0], of[..., 1], of[..., 2]
    fx, fy, fz = 1 - cx, 1 - cy, 1 - cz
    w = np.stack([cx * cy * cz, cx * fy * cz, fx * fy * cz, fx * cy * cz, cx * cy * fz, cx * fy * fz, fx * fy * fz,
                  fx * cy * fz], -1)
    with np.errstate(invalid="ignore"):
        interp = (w * c.table.astype(np.float64)[idx, 0]).sum(-1)
    rw = 1.0 / np.maximum(2.0 * scal.astype(np.float64)[None, :] * std.reshape(-1, 1), 1.0)
    lf = interp * rw
    dec = c.dec.astype(np.float64)[0]
    return Forward(pos, mag.reshape(-1), xcb.reshape(-1), std.reshape(-1), idx, w, interp, rw, lf, lf @ dec,
                   np.abs(lf * dec).sum(-1))


def rtol_rw(c, fwd):
    """[N, 1]: relative bound on the kernels' `interp * rescale_weight` against interp * rw64, from one-ulp (E = 2^-23)
    v_log_f32 / v_exp_f32 / v_rcp_f32 and half-ulp (U = 2^-24) roundings of everything else.

    fast_cbrt(x) = exp2(log2(x) * fp32(1/3)): the logarithm is off by E |log2 x|, the constant and the product by U each, so
    the exponent is off by (E + 2 U) |log2 x| / 3 = 2 E |log2 x| / 3, which exp2 turns into a relative ln 2 times that; exp2
    itself adds E:                       cbrt_err(x) = 2 ln2 E |log2 x| / 3 + E.
    x = (area * (t * t)) * dist carries two roundings (t * t is exact here): 2 U / 3 after the cube root.  The divisions by
    static_scale and 4 are exact.  Past the contraction boundary std is multiplied by sc^2, sc = fast_cbrt(2 cm - 1) / cm
    (2 cm - 1 is exactly 1 or 3 here): 2 (cbrt_err(2 cm - 1) + U) + U for the square, + U for the product.  Then
    (scal * 2) * std: U; fmaxf: exact; v_rcp_f32: E; the product with the (exact) interpolated feature: U.  Where the maximum
    is 1 on either side the bound still holds: the function is continuous and the weight is then exactly 1."""
    def cbrt_err(x):
        return 2 * np.log(2) * E * np.abs(np.log2(x)) / 3 + E

    r = cbrt_err(fwd.xcb) + 2 * U / 3
    cm = np.maximum(fwd.mag, 1.0)
    r = r + np.where(fwd.mag < 1, 0.0, 2 * (cbrt_err(2 * cm - 1) + U) + 2 * U)
    return (r + U + E + U)[:, None]


def logit_err(c, fwd):
    """[N]: absolute error of the fp32 logit against x -- one product and one addition rounding per level"""
    return 2 * c.L * U * fwd.ax


def density_bound(c, fwd):
    """[N]: |density - exp(x)| <= exp(x) (2 ulp of expf + the logit's error)"""
    return np.exp(fwd.x) * (2 * E + logit_err(c, fwd))


def gx_rtol(c, fwd):
    """[N]: relative bound on g exp(clip(log(density), -15, 15)) against g exp(clip(x, -15, 15)): expf, logf, expf at two ulp
    each -- the logarithm's scaled by |x| -- and, where the clamp lets the logit through, the forward logit's own error"""
    xc = np.clip(fwd.x, -15, 15)
    err = logit_err(c, fwd)
    return (3 + np.abs(xc)) * 2 * E + np.where(np.abs(fwd.x) <= 15 + err, err, 0.0)


@dataclass
class Backward:
    gx: np.ndarray  # [N]
    ddec: np.ndarray  # [L]
    ddec_bound: np.ndarray  # [L]
    table: np.ndarray  # [L * T]
    a: np.ndarray  # [L * T] sum of |terms|
    nt: np.ndarray  # [L * T] terms of samples that send records (g != 0)
    touched: np.ndarray  # [L * T] bool: some sample's corner, silent or not
    soft: np.ndarray  # [L * T] sum of |terms| * the terms' relative error (gx, and rw where given)
    recs: np.ndarray
    tmax: np.ndarray
    amax: np.ndarray
    ts: int

    def atomic_bound(self):
        """per entry: the terms' own error + (terms + 8) roundings on the sum of |terms|"""
        return self.soft + (self.nt + 8) * U * self.a


def backward_ref(c, fwd, g, clip=15.0, use_rw=True, dec_shift=0, rw_rtol=None):
    """float64 backward from the exact logit.  clip / use_rw / dec_shift: the right values, or a wrong variant's (a clamp
    elsewhere, the rescale weight left out of the table term, dec_l taken from level l + dec_shift).  rw_rtol: rtol_rw of a
    rescaled case, added to every term's relative error."""
    L, T = c.L, 1 << LOG2_T
    g = np.asarray(g, np.float64).reshape(-1)
    gx = g * np.exp(np.clip(fwd.x, -clip, clip))  # np.clip keeps a NaN, as torch.clamp does
    rel = gx_rtol(c, fwd)[:, None]  # [N, 1]
    if rw_rtol is not None:  # the weight's error in the term itself, and through every feature in the forward's logit
        rel = rel + rw_rtol + rw_rtol * fwd.ax[:, None]
    with np.errstate(invalid="ignore"):
        dterm = gx[:, None] * fwd.lf
        ddec = dterm.sum(0)
        a_dec = np.abs(dterm).sum(0)
        ddec_bound = (np.abs(dterm) * rel).sum(0) + (len(g) + 8) * U * a_dec
        dec = np.roll(c.dec.astype(np.float64)[0], -dec_shift)
        genc = gx[:, None] * dec[None, :] * (fwd.rw if use_rw else 1.0)  # [N, L]
        terms = fwd.w * genc[..., None]  # [N, L, 8]
        size = L * T
        key = fwd.idx.reshape(-1)
        table = np.bincount(key, terms.reshape(-1), size)
        a = np.bincount(key, np.abs(terms).reshape(-1), size)
        soft = np.bincount(key, (np.abs(terms) * rel[..., None]).reshape(-1), size)
    live = g != 0
    nt = np.bincount(key, np.broadcast_to(live[:, None, None], terms.shape).reshape(-1).astype(np.float64), size)
    touched = np.bincount(key, minlength=size) > 0
    ts = log2_slice(L, 1, LOG2_T)
    ent = fwd.idx - (np.arange(L) * T)[None, :, None]
    sl = (np.arange(L)[None, :, None] << (LOG2_T - ts)) + (ent >> ts)
    recs = np.bincount(sl[live].reshape(-1), minlength=L << (LOG2_T - ts)).astype(np.float64)
    fin = np.nan_to_num(np.abs(terms), nan=0.0, posinf=0.0)
    tmax = fin.reshape(len(g), L, -1).max((0, 2)) if len(g) else np.zeros(L)
    amax = np.nan_to_num(a, nan=0.0, posinf=0.0).reshape(L, -1).max(1)
    return Backward(gx, ddec, ddec_bound, table, a, nt, touched, soft, recs, tmax, amax, ts)


# ---- the level-partitioned forward's launch arithmetic (hashgrid.hip: nrhip_proposal_density_fwd) --------------------------
def lp_plan(n, L):
    """-> (per_quarter, blocks_per_unit, units, blocks)"""
    per_quarter = ((n + 3) // 4 + 255) // 256 * 256
    bpu = per_quarter // 256
    units = 4 * L
    return per_quarter, bpu, units, 8 * ((units + 7) // 8) * bpu


def lp_writes(n, L, variant=None):
    """[L, n] how often proposal_levels_lp_kernel writes each (level, sample), block by block as the kernel maps them.
    variant: None, or a wrong kernel -- "hi-1": a quarter's upper end one short; "drop-first": the first sample of a quarter
    left to the previous one; "unit-round": the units of an incomplete last round of 8 dropped"""
    per_quarter, bpu, units, blocks = lp_plan(n, L)
    count = np.zeros((L, n), np.int64)
    for b in range(blocks):
        xcd, q = b & 7, b >> 3
        unit = xcd + 8 * (q // bpu)
        if unit >= units or (variant == "unit-round" and unit >= units // 8 * 8):
            continue
        l, quarter = divmod(unit, 4)
        lo = quarter * per_quarter + (q % bpu) * 256
        hi = min((quarter + 1) * per_quarter, n) - (1 if variant == "hi-1" else 0)
        i = np.arange(lo, lo + 256)
        if variant == "drop-first":
            i = i[(i != quarter * per_quarter) | (quarter == 0)]
        i = i[i < hi]
        count[l, i] += 1
    return count


# ---- the decoder-gradient kernel's grid-stride loop (hashgrid.hip: proposal_decoder_grad_kernel) ----------------------------
def stride_case(n, L, vec, seed=0):
    """Inputs of the binned backward for which d dec_l is a short exact sum: density 1 (the caller sets the decoder weight to
    0), level features small integers, g a small non-zero integer at no more than 64 samples -- the first and last sample of
    both passes of the 1024-block grid, both sides of a block edge in each pass, and a few others -- and 0 elsewhere.
    vec: 4 or 1, the samples per thread of the instantiation the shape reaches.  -> (lf [L, n] fp32, g [n] fp32, the chosen
    samples, d dec [L] float64, exact)"""
    per_pass = 1024 * 256 * vec
    assert per_pass < n < 2 * per_pass
    rng = np.random.default_rng([seed, n, L])
    edge = 256 * vec
    chosen = np.unique(np.r_[0, per_pass - 1, per_pass, n - 1, edge - 1, edge, per_pass + edge - 1, per_pass + edge,
                             rng.integers(0, per_pass, 24), rng.integers(per_pass, n, 24)])
    assert len(chosen) <= 64
    g = np.zeros(n, np.float32)
    g[chosen] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], len(chosen))
    lf = np.empty((L, n), np.float32)
    for lo in range(0, n, 1 << 18):  # in chunks: the integers of a chunk depend on its position alone
        hi = min(lo + (1 << 18), n)
        lf[:, lo:hi] = np.random.default_rng([seed, L, lo]).integers(-4, 5, (L, hi - lo))
    ddec = (lf[:, chosen].astype(np.float64) * g[chosen].astype(np.float64)).sum(1)
    return lf, g, chosen, ddec


# ---- special cases of the backward ------------------------------------------------------------------------------------------
def saturation_case(n=2049, L=6, seed=0):
    """A hot decoder row, weights +-16 alternating over the levels, and every eighth ray standing still on a point whose
    coordinates are multiples of 4 (all offsets 0: its features are table entries, its logit a multiple of 16).  The logits
    then cover (-15, 15), both sides of +-15, +-16, 0 exactly, and beyond +-88 and +-104: densities of inf, subnormal and 0."""
    c = exact_case(n, L, seed)
    rng = np.random.default_rng([seed, n, L, 2])
    still = np.arange(c.R) % 8 == 0
    o, d = c.o.copy(), c.d.copy()
    o[still] = 4.0 * rng.integers(-1, 2, (int(still.sum()), 3))
    d[still] = 0.0
    dec = (16.0 * (-1.0) ** np.arange(L)).astype(np.float32)[None, :]
    return replace(c, o=o, d=d, dec=dec)


def saturation_grad(fwd, seed=0):
    """g: non-zero multiples of 1/8, exactly 0 at every other sample whose density overflows (inf * 0 must not appear)"""
    rng = np.random.default_rng([seed, len(fwd.x), 3])
    g = rng.choice(np.r_[-8:0, 1:9], len(fwd.x)) / 8.0
    hot = np.flatnonzero(fwd.x > 89)
    g[hot[::2]] = 0.0
    return g.astype(np.float32)


def nan_case(n, L=6, seed=0, level=0):
    """the exact case with ONE table entry NaN: the level's most shared one.  -> (case, the samples whose density is NaN:
    those with that entry among their 8 corners, whatever its weight -- 0 * NaN is NaN in the reference's lerp too)"""
    c = exact_case(n, L, seed)
    idx = forward_ref(c).idx
    row = int(np.argmax(np.bincount(idx[:, level, :].reshape(-1), minlength=L << LOG2_T)))
    table = c.table.copy()
    table[row] = np.nan
    return replace(c, table=table), np.flatnonzero((idx[:, level, :] == row).any(-1))


def grad_with_silent_windows(n, seed=0):
    """g: non-zero multiples of 1/8, exactly 0 over the whole aligned 64-sample windows 1 and 3 (where n reaches them), over
    the second half of window 0 and over the first 7 samples of window 2, and +-0 mixed"""
    rng = np.random.default_rng([seed, n, 4])
    g = rng.choice(np.r_[-8:0, 1:9], n) / 8.0
    for lo, hi in ((64, 128), (192, 256), (32, 64), (128, 135)):
        g[lo:hi] = 0.0
    g[72:80] = -0.0
    return g.astype(np.float32)
