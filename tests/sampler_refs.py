"""The sharp-weight input families of the PDF resampler and the float64 references its kernels are held to, element by
element (tests/test_sampler_refs_host.py on the CPU, tests/test_gpu_sampler_sharp.py on the GPU).

The inverse CDF amplifies the fp32 rounding of the CDF by (bin width / pdf mass), so a new bin cannot be compared with ONE
reference value: two correct summation orders differ by more than a wrong kernel does on smooth weights.  Instead every
new bin is held to a BRACKET.  With C the float64 CDF, u_i the exact query point and F^-1 the float64 piecewise-linear
inverse with the reference's semantics (searchsorted side="right", indices clipped, nan -> 0, t clipped to [0, 1]), which
is monotone in u, any fp32 evaluation of C and u perturbs every difference u - C[j] by at most DELTA, so

    F^-1(max(u_i - DELTA, 0)) - eps_b  <=  new bin i  <=  F^-1(min(u_i + DELTA, 1)) + eps_b.

(If C_k[j] <= u_k in fp32 then C[j] <= u + DELTA, and if C[j] <= u - DELTA then C_k[j] <= u_k: the fp32 bin index lies
between the two exact ones; inside one bin t_k = N_k / (N_k + M_k) with N_k <= N + DELTA and M_k >= M - DELTA is at most
the exact t at u + DELTA, and symmetrically.  The clamps at 0 and 1 hold because fp32 queries and CDFs never leave [0, 1];
they make u = 0 exactly on a CDF that starts flat a sharp case.)  DELTA, eps_b and the euclidean bound are derived below, next
to their constants; nothing here is fitted to a kernel's output.

Measured, for the record only (no threshold is set from these).  On the CPU, worst element of all cases: the share of DELTA
that |F(got) - u| uses is 0.038 for the oracle's pdf_sample, 0.16 with a sequential fp32 running sum, 0.059 with a pairwise
one; the oracle's fp32 Spacing lies within 0.22 of the euclidean bound's width (lam = 0.5; 0.13 at lam = -1); the C oracle's
first-round weights differ from the numpy oracle's by 0.12 of the stage-2 bound on the unscaled field, 0.002 on the sharp one.

On an MI355X (tests/test_gpu_sampler_sharp.py, worst err / bound over all cases of a stage):
  ops.pdf_sample          share of DELTA 0.038 (7 -> 130; 0.013 at 64 -> 32, 0.0011 at 512 -> 512), euclidean 0.15
  ops.power_sampler       spacing bins bit for bit; euclidean 0.075 (lam = -1) ... 0.10 (lam = 0.5)
  fused sampler, stage 1  bit for bit ops.power_sampler's; euclidean 0.12
                 stage 2  weights 0.0089 at 13 rays (48 -> 96 -> 7, L = 4), 0.023 at 8229 rays
                 stage 3  share of DELTA 0.021 at 13 rays, 0.067 at 8229 rays; euclidean 0.15
                 actors   both NRHIP_SAMPLER_ACTOR_INLINE settings: share of DELTA 0.012, euclidean 0.14
  unfused chain           density |got / oracle - 1| / rho 0.016; weights, bins and euclidean as the fused kernel
  fused against unfused   final euclidean bins identical bit for bit (difference / sum of the two bounds = 0)
Before the exclusive transmittance sum of the fused kernel stopped being `inclusive - own term`, its stage-2 weights
missed the bound by up to 28 x (w = 1.0 for 0.99912) and 480 x (0.135 for 0.199) on the OPAQUE field."""
import itertools

import numpy as np

import neurad_oracle as O
import sharp_refs
import synth
from conftest import load_golden

U = 2.0 ** -24  # fp32 unit roundoff
ONE_BELOW = np.float32(1.0 - 2.0 ** -24)  # the largest fp32 below 1
R = 13  # not a multiple of the 4 rays per workgroup
COUNTS = [(128, 64), (64, 32), (63, 64), (65, 33), (130, 65), (7, 130), (1, 1), (512, 512)]  # (Sp, Sn)
PADS = [0.01, 0.0]  # histogram_padding; 0: the eps branch on the empty ray, flat CDF stretches on the one-hot rays
RANDS = ["none", "single", "perbin"]
EPS = np.float64(np.float32(1e-5))  # the resampler's eps as the kernels hold it


def f64(a):
    return np.asarray(a, np.float64)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def sharp_weights(Sp, seed, R=R):
    """[R, Sp] weights whose rows cycle through: one-hot at the first / last / a middle bin, two neighbouring bins
    (0.6 / 0.4), empty, heavy-tailed (uniform^8, normalised), smooth (uniform(0, 0.2)), exact ties, the whole mass
    1 - 2^-24 in the first bin and 2^-24 in the last, then a one-hot and a two-bin row at the 64-weight chunk boundary"""
    w = np.zeros((R, Sp), np.float32)
    last, mid = Sp - 1, Sp // 2
    edge = 63 if Sp > 64 else max(Sp // 2 - 1, 0)  # the last weight of the first chunk, where there is a second one
    for r in range(R):
        k = r % 13
        if k == 0:
            w[r, 0] = 1.0
        elif k == 1:
            w[r, last] = 1.0
        elif k == 2:
            w[r, mid] = 1.0
        elif k == 3:
            w[r, min(Sp // 3, max(Sp - 2, 0))] = 0.6
            if Sp > 1:
                w[r, min(Sp // 3, Sp - 2) + 1] = 0.4
        elif k == 4:
            pass
        elif k in (5, 9):
            h = synth.uniform((Sp,), 0.0, 1.0, seed + r).astype(np.float64) ** 8
            w[r] = (h / h.sum()).astype(np.float32)
        elif k in (6, 10):
            w[r] = synth.uniform((Sp,), 0.0, 0.2, seed + r)
        elif k == 7:
            w[r] = np.float32(0.37)
        elif k == 8:
            w[r, last] = np.float32(2.0 ** -24)
            w[r, 0] = ONE_BELOW if Sp > 1 else np.float32(1.0)
        elif k == 11:
            w[r, edge] = 1.0
        else:
            w[r, edge] = 0.6
            w[r, min(edge + 1, last)] += np.float32(0.4)
    return w


def sharp_rand(kind, Sn, seed, R=R):
    """None | single jitter [R] | per-bin jitter [R, Sn + 1], in [0, 1), with exactly 0.0 and exactly 1 - 2^-24 among them
    (0.0 on a one-hot ray whose CDF starts flat: the first query is u = 0 exactly)"""
    if kind == "none":
        return None
    if kind == "single":
        r = np.minimum(synth.uniform((R,), 0.0, 1.0, seed), ONE_BELOW)
        r[0], r[1 % R], r[2 % R], r[3 % R] = 0.0, ONE_BELOW, 0.0, ONE_BELOW
        return r
    r = np.minimum(synth.uniform((R, Sn + 1), 0.0, 1.0, seed), ONE_BELOW)
    r[0, 0], r[1 % R, -1], r[2 % R, 0], r[3 % R, Sn // 2] = 0.0, ONE_BELOW, 0.0, ONE_BELOW
    r[min(6, R - 1)] = 0.0  # a smooth ray with every query at u = i / nb
    return r


def make_case(Sp, Sn, pad, rand_kind, with_nears, far, seed=7, R=R, jittered_bins=False):
    """one resampling case: fp32 inputs as numpy arrays (nears / rand may be None)"""
    nears = synth.uniform((R,), 0.5, 3.0, seed + 100) if with_nears else None
    fars = np.full((R,), far, np.float32)
    if jittered_bins:
        g = load_golden("sampler_train")
        assert Sp == g["sp0"].shape[1] - 1
        bins = np.ascontiguousarray(g["sp0"][np.arange(R) % g["sp0"].shape[0]])
    else:
        bins = np.ascontiguousarray(O.power_sampler(np.zeros(R), fars, Sp)[0])
    return dict(w=sharp_weights(Sp, seed, R), bins=bins, Sn=Sn, pad=pad, rand=sharp_rand(rand_kind, Sn, seed + 50, R),
                nears=nears, fars=fars, lam=-1.0, scaling=0.1,
                name=f"{Sp}->{Sn} pad={pad} rand={rand_kind} nears={with_nears} far={far}" + (" jittered" * jittered_bins))


def cases(counts=None):
    """every case of one count pair (or of all): pads x jitters x nears x fars, plus the jittered existing bins once"""
    for (Sp, Sn), pad, rk, wn, far in itertools.product(COUNTS if counts is None else [counts], PADS, RANDS, (False, True),
                                                        (200.0, 20000.0)):
        yield make_case(Sp, Sn, pad, rk, wn, far)
    if counts is None or counts == (128, 64):
        yield make_case(128, 64, 0.01, "perbin", True, 200.0, jittered_bins=True)
        yield make_case(128, 64, 0.0, "single", False, 20000.0, jittered_bins=True)


# ---- the bracket ------------------------------------------------------------------------------------------------------
def delta(Sp):
    """Worst-case fp32 perturbation of u - C[j], C in [0, 1], to first order in u = 2^-24 (gamma_n = n u / (1 - n u)):
      each pdf term (w + pad + add) / tot: 3 roundings (the two additions, the division) ................. 3
      tot, a sum of Sp non-negative terms in ANY order, plus `tot += padding` ........................... Sp
        (on the eps branch tot's error returns through padding = eps - tot: Sp u tot spread over the terms, while
         tot + padding itself is eps to 2 u -- no more than the Sp counted here)
      the running sum of at most Sp such terms, any order (sequential, pairwise, wave scan + chunk carry) . Sp - 1
      u_i: 1/nb, 1 - 1/nb, the linspace step, its product with i (or end - step * j), rand / nb, the sum .. 6
      slack for the eps branch (padding's own rounding, the add of `add` counted above only once) ......... 4
    -> (2 Sp + 12) u, relative to values <= 1.  min(1, .) only moves a CDF entry towards its exact value's range.
    The float64 evaluation of C and u adds ~Sp 2^-53: 2^-40 covers it."""
    n = 2 * Sp + 12
    return n * U / (1 - n * U) + 2.0 ** -40


def cdf64(w, pad):
    """the resampler's CDF C[0 .. Sp] in float64 from fp32 weights (ray_samplers.py:318-331)"""
    w = f64(w) + np.float64(np.float32(pad))
    tot = w.sum(-1, keepdims=True)
    padding = np.maximum(EPS - tot, 0.0)
    pdf = (w + padding / w.shape[-1]) / (tot + padding)
    c = np.minimum(1.0, np.cumsum(pdf, -1))
    c[..., -1] = 1.0  # exact: the pdf sums to one
    return np.concatenate([np.zeros_like(c[..., :1]), c], -1)


def queries64(Sn, rand, R):
    """the exact query points: linspace(0, 1 - 1/nb, nb)[i] = i / nb, plus 1 / (2 nb) or rand / nb (ray_samplers.py:333-345)"""
    nb = Sn + 1
    i = np.arange(nb, dtype=np.float64)[None, :]
    if rand is None:
        return np.broadcast_to((i + 0.5) / nb, (R, nb))
    rand = f64(rand).reshape(R, -1)
    return (i + rand) / nb


def inverse_cdf(C, bins, u):
    """F^-1 with the reference's semantics (ray_samplers.py:347-366) in float64 -> (value, upper edge of the bin used)"""
    Sp = C.shape[-1] - 1
    inds = (C[:, None, :] <= u[:, :, None]).sum(-1)  # searchsorted(side="right")
    below, above = np.clip(inds - 1, 0, Sp), np.clip(inds, 0, Sp)
    c0, c1 = np.take_along_axis(C, below, -1), np.take_along_axis(C, above, -1)
    b0, b1 = np.take_along_axis(bins, below, -1), np.take_along_axis(bins, above, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (u - c0) / (c1 - c0)
    t = np.clip(np.nan_to_num(t, nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0, 1.0)
    return b0 + t * (b1 - b0), b1


def bracket(w, bins, Sn, pad, rand):
    """-> (lo, hi, centre) [R, Sn + 1] for the new spacing bins.  eps_b, the rounding of the final lerp
    b0 + t (b1 - b0) with t = (u - c0) / (c1 - c0): three roundings in t (<= 1), one each in b1 - b0, the product and the
    sum -> at most 6 u times the upper edge of the bin (bins are >= 0 and ascending); the perturbation of u - c0 itself is
    DELTA's business."""
    w, bins = np.asarray(w, np.float32), f64(bins)
    R, Sp = w.shape
    C, u, d = cdf64(w, pad), queries64(Sn, rand, R), delta(Sp)
    lo, _ = inverse_cdf(C, bins, np.maximum(u - d, 0.0))
    hi, top = inverse_cdf(C, bins, np.minimum(u + d, 1.0))
    mid, _ = inverse_cdf(C, bins, np.clip(u, 0.0, 1.0))
    eps_b = 6 * U * np.abs(top)
    return lo - eps_b, hi + eps_b, mid


def assert_sharp(lo, hi, Sn, what):
    """a wide bracket checks nothing: in every case at least 99 % of the elements are narrower than 1 / (4 Sn), a quarter
    of the mean new-bin width"""
    narrow = float(((hi - lo) < 1.0 / (4 * Sn)).mean())
    assert narrow >= 0.99, f"{what}: only {100 * narrow:.2f} % of the brackets are narrower than 1/(4*{Sn})"
    return narrow


def check_bracket(got, lo, hi, what, centre=None):
    """every element inside its bracket; -> max |got - centre| / (hi - lo), for the record (euclidean bounds)"""
    got = f64(got)
    assert got.shape == lo.shape, (got.shape, lo.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite at {np.argwhere(~np.isfinite(got))[:5].tolist()}"
    off = (got < lo) | (got > hi)
    if off.any():
        k = tuple(np.argwhere(off)[0])
        raise AssertionError(f"{what}: {int(off.sum())} elements outside their bracket, first {k}: got {got[k]!r} "
                             f"bracket [{lo[k]!r}, {hi[k]!r}]")
    if centre is None:
        return 0.0
    return float((np.abs(got - centre) / np.maximum(hi - lo, 1e-300)).max())


def delta_used(got, w, bins, Sn, pad, rand):
    """for the record: the share of DELTA a result needs, max |F(got) - u| / DELTA with F the float64 CDF as a function of
    the bin position (got moved by up to eps_b towards F^-1(u) first: the lerp's rounding is not DELTA's)"""
    w, bins, got = np.asarray(w, np.float32), f64(bins), f64(got)
    R, Sp = w.shape
    C, u = cdf64(w, pad), np.clip(queries64(Sn, rand, R), 0.0, 1.0)
    mid, top = inverse_cdf(C, bins, u)
    eps_b = 6 * U * np.abs(top)
    g = got - np.clip(got - mid, -eps_b, eps_b)
    worst = 0.0
    for r in range(R):
        strict = np.concatenate([[True], np.diff(bins[r]) > 0])  # zero-width bins: F jumps there, either value is right
        F = np.interp(g[r], bins[r][strict], C[r][strict])
        jump = np.isin(g[r], bins[r])  # on an existing edge F^-1 may jump (a flat stretch of C): any u of the stretch maps here
        worst = max(worst, float(np.where(jump, 0.0, np.abs(F - u[r])).max()))
    return worst / delta(Sp)


def check_monotone(got, what):
    """new bins non-decreasing per ray up to eps_b (6 u times the bin)"""
    g = f64(got)
    drop = g[:, :-1] - g[:, 1:]
    bad = drop > 6 * U * np.abs(g[:, :-1])
    assert not bad.any(), f"{what}: bins decrease at {np.argwhere(bad)[:5].tolist()}"


def check_case_bins(case, got_sp, what=None):
    """the new spacing bins of `case` against the bracket and the 99 % condition -> (ratio, share of narrow brackets)"""
    what = what or case["name"]
    lo, hi, mid = bracket(case["w"], case["bins"], case["Sn"], case["pad"], case["rand"])
    narrow = assert_sharp(lo, hi, case["Sn"], what)
    check_bracket(got_sp, lo, hi, what + ": spacing bins")
    check_monotone(got_sp, what)
    return delta_used(got_sp, case["w"], case["bins"], case["Sn"], case["pad"], case["rand"]), narrow


# ---- euclidean bins ---------------------------------------------------------------------------------------------------
def _power64(x, lam):
    if lam == 1:
        return x
    if lam == 0:
        return np.log1p(x)
    l1 = abs(lam - 1)
    return (l1 / lam) * ((x / l1 + 1) ** lam - 1)


def _inv_power64(a, lam):
    """-> (value, pow before the `- 1`, base) of the inverse power transform"""
    if lam == 1:
        return a, np.abs(a), np.ones_like(a)
    if lam == 0:
        return np.expm1(a), np.exp(a), np.ones_like(a)
    l1 = abs(lam - 1)
    base = np.maximum(a * lam / l1 + 1, 1e-10)
    p = base ** (1.0 / lam)
    return (p - 1) * l1, p, base


def euclid_bounds(sp, nears, fars, lam=-1.0, scaling=0.1):
    """to_euclid(b) = inv_power_fn(b s_far + (1 - b) s_near, lam) / scaling at the kernel's OWN spacing bins `sp`, in
    float64, with the fp32 evaluation's error propagated per element -> (lo, hi, centre).

    The argument a = b s_far + (1 - b) s_near carries
      eps_a = b e_far + (1 - b) e_near + u (|b s_far| + 2 |(1 - b) s_near| + |a|):
      the roundings of b s_far, of 1 - b and of its product with s_near, and of the sum (with FMA contraction: fewer);
      e_near, e_far = (3 |lam| + 7) u m, the error of s = power_fn(x scaling): `x scaling`, `/ lam_1`, `+ 1` perturb the
        base of the power by 3 u, i.e. the power by 3 |lam| u; the power itself 4 u (a correctly rounded reciprocal for
        lam = -1, else a 2-ulp powf and the rounded exponent); `- 1`, the rounded constant lam_1 / lam and the product: 3
        more.  They are relative to the magnitude BEFORE the cancelling `- 1`, m = (lam_1 / |lam|) max(pow, 1), not to |s|
        (lam = 0, 1: m = |s|).  A near plane of exactly 0 gives s_near = 0 exactly (0 / lam_1 + 1 = 1, 1^lam = 1, 1 - 1 = 0).
    Through the inverse: the base a lam / lam_1 + 1 adds 2 u |a| and u |base| lam_1 / |lam| in units of a; the value is
    evaluated in float64 at both ends of that interval (the map is monotone), which is where one ulp of the argument becomes
    ~1e-4 relative at the far end for lam = -1 and far = 20000 (base ~ 1 / 1001); then the power's own
    (4 + |ln(base) / lam|) u relative to the power (before its `- 1`), and `- 1`, `* lam_1`, `/ scaling`: 3 u of the result."""
    sp = f64(sp)
    R = sp.shape[0]
    sc = np.float64(np.float32(scaling))
    near = np.zeros((R, 1)) if nears is None else f64(nears).reshape(R, 1)
    far = f64(fars).reshape(R, 1)
    s_near, s_far = _power64(near * sc, lam), _power64(far * sc, lam)
    if lam in (0, 1):
        m_near, m_far = np.abs(s_near), np.abs(s_far)
    else:
        l1 = abs(lam - 1)
        m_near = (l1 / abs(lam)) * np.maximum((near * sc / l1 + 1) ** lam, 1.0)
        m_far = (l1 / abs(lam)) * np.maximum((far * sc / l1 + 1) ** lam, 1.0)
    k_s = (3 * abs(lam) + 7) * U
    e_near, e_far = np.where(near == 0, 0.0, k_s * m_near), k_s * m_far
    a = sp * s_far + (1 - sp) * s_near
    eps_a = (np.abs(sp) * e_far + np.abs(1 - sp) * e_near
             + U * (np.abs(sp * s_far) + 2 * np.abs((1 - sp) * s_near) + np.abs(a)))
    if lam not in (0, 1):
        l1 = abs(lam - 1)
        base = a * lam / l1 + 1
        eps_a = eps_a + (2 * U * np.abs(a) + U * np.abs(base) * l1 / abs(lam))  # the base's own roundings, as argument error
    mid, _, _ = _inv_power64(a, lam)
    ends = []
    for s in (-1.0, 1.0):
        v, p, base = _inv_power64(a + s * eps_a, lam)
        l1 = 1.0 if lam in (0, 1) else abs(lam - 1)
        k = 4 + (0.0 if lam in (0, 1) else np.abs(np.log(base) / lam))
        ends.append((v, k * U * p * l1 + 3 * U * np.abs(v)))
    lo = np.minimum(ends[0][0] - ends[0][1], ends[1][0] - ends[1][1]) / sc
    hi = np.maximum(ends[0][0] + ends[0][1], ends[1][0] + ends[1][1]) / sc
    return lo, hi, mid / sc


def check_euclid(got_eu, sp, nears, fars, what, lam=-1.0, scaling=0.1):
    lo, hi, mid = euclid_bounds(sp, nears, fars, lam, scaling)
    return check_bracket(got_eu, lo, hi, what + ": euclidean bins", mid)


# ---- the fused sampler's proposal fields and its weights --------------------------------------------------------------
SHARP = 12.0  # decoder scale of the sharp fields, chosen on the CPU from the oracle's densities (4, 8, 12, 16 tried): the
#               smallest at which log-densities pass +-15 along the rays of sharp_rays() and more than a third of the rays
#               put > 0.9 of their weight into one bin (tests/test_sampler_refs_host.py asserts both)
OPAQUE = 20.0  # a wall: log-densities to +-30, density x bin length up to ~1e7, orders of magnitude past exp's range -- the
#                family sharp_refs.sharp_bins holds the compositing kernels to (sigma * delta past 88)


def sharp_rays(R, seed=21):
    o, d, area, _ = synth.rays(R, seed)
    return o, d, area


def sharp_prop(seed, L=6, factor=SHARP, lg=11, half=False):
    """builders.prop_params's field (L = 6: the same table and decoder) with the decoder scaled by `factor`: a trained
    proposal field's range of densities.  half: fp16 table storage -- the oracle sees the rounded table"""
    w, _ = synth.linear(1, L, seed + 1, bias=False)
    table = synth.hash_table(L * 2**lg, 1, seed=seed, scale=2.0)
    if half:
        table = table.astype(np.float16).astype(np.float32)
    return O.ProposalParams(O.GridParams(table, L, 128, 4096, lg), 100.0, ((w + np.float32(0.3)) * np.float32(factor)))


def prop_rho(p):
    """Relative difference of two fp32 evaluations of density = exp(sum_l (v_l rw_l) dec_l) at bit-identical contracted
    positions (the kernels round the position arithmetic op for op like the reference, csrc/common.h), in units of u:
      v_l, the trilinear blend of 8 corners of magnitude <= tmax: three levels of a o + b (1 - o), 4 roundings each (an
        fma saves one) -> 12 u tmax per evaluation, 24 between two
      rw_l = 1 / max(1, 2 s_l std) <= 1, relative: std through two cube roots -- the kernels' exp2(log2(x) / 3) on 1-ulp
        v_log_f32 / v_exp_f32 is 2 u |log2 x| / 3 + u |log2 x| / 3 absolute in the exponent, |log2 x| <= 64, times ln 2,
        plus an ulp: 46 u; the contraction's second root has |log2| <= 8 and is squared: 20 u; the reference's two powers,
        the square and the products 8 u; 2 s std, the reciprocal (1 ulp against a rounded division) 6 u -> 80
      the two products: 2 u per evaluation -> 4
      the sum of L terms, any order: (L - 1) u sum |term| per evaluation -> 2 (L - 1)
    -> |d log density| <= (108 + 2 (L - 1)) u tmax sum_l |dec_l|, and the exponentials (2 ulp and 1 ulp) 6 u."""
    L = p.grid.num_levels
    tmax = float(np.abs(p.grid.table).max())
    return (108 + 2 * (L - 1)) * U * tmax * float(np.abs(p.decoder_w).sum()) + 6 * U


def weights_ref(eu, dens32, rho):
    """cameras/rays.py:188-210 in float64 from the fp32 edges and the oracle's fp32 densities -> (w, bound): the
    per-element bound of sharp_refs.ref_density for the transmittance sum and the alpha, widened by the weight's
    sensitivity to a relative density error rho: dw = rho (sd e^-sd T + alpha T sum_{j<i} sd_j)"""
    eu = np.asarray(eu, np.float32)
    delta32 = eu[:, 1:] - eu[:, :-1]  # one correctly rounded subtraction, as every evaluation forms it
    w, Tn, an, _, fscale, _ = sharp_refs.ref_density(delta32, dens32, np.zeros_like(delta32))
    sd = f64(dens32) * f64(delta32)
    cex = np.concatenate([np.zeros_like(sd[:, :1]), np.cumsum(sd, -1)[:, :-1]], -1)
    return w, sharp_refs.TINY + fscale + rho * Tn * (sd * np.exp(-sd) + an * cex)


def check_weights(got_w, eu, dens32, rho, what):
    w, bound = weights_ref(eu, dens32, rho)
    sharp_refs.check(got_w, w, bound, what + ": weights")
    return float((np.abs(f64(got_w) - w) / bound).max())


# (counts, level counts per round, fp16 table, nears, fars: None | "below" | "above" the sky distance, padding, decoder scale)
VARIANTS = [
    ((128, 64, 32), (6, 6), False, False, None, 0.01, SHARP),
    ((128, 64, 32), (6, 6), False, True, "below", 0.0, SHARP),
    ((128, 64, 32), (6, 6), False, False, None, 0.01, 1.0),      # the unscaled field of the golden tests
    ((130, 65, 33), (6, 6), True, False, "above", 0.01, SHARP),
    ((48, 96, 7), (4, 4), False, True, None, 0.0, SHARP),
    ((300, 70, 33), (8, 8), False, False, "below", 0.01, SHARP),
    ((64, 16), (5,), False, True, "above", 0.01, SHARP),       # one round, generic level count
    ((128, 64, 32), (6, 4), False, False, None, 0.0, SHARP),   # rounds with different level counts: the lt = 0 path
    ((130, 65, 33), (5, 5), True, True, "below", 0.0, SHARP),
    ((300, 70, 33), (6, 6), True, True, None, 0.01, SHARP),
    ((48, 96, 7), (8, 8), True, False, "above", 0.01, SHARP),
    ((64, 16), (6,), False, False, None, 0.0, SHARP),
    ((128, 64, 32), (6, 6), False, False, None, 0.01, OPAQUE),
    ((128, 64, 32), (6, 6), False, True, None, 0.0, OPAQUE),
    ((130, 65, 33), (6, 6), True, True, "below", 0.01, OPAQUE),
]


def variant_inputs(R, with_nears, fars_kind):
    """-> origins, directions, pixel areas, nears | None, fars | None"""
    o, d, area = sharp_rays(R)
    nears = synth.uniform((R,), 0.5, 3.0, 107) if with_nears else None
    fars = None if fars_kind is None else np.full(R, 200.0 if fars_kind == "below" else 30000.0, np.float32)
    return o, d, area, nears, fars


def variant_props(levels, half, factor):
    return [sharp_prop(91 + 4 * k, L=L, factor=factor, half=half) for k, L in enumerate(levels)]


VARIANT_IDS = [f"{'-'.join(map(str, v[0]))}_L{''.join(map(str, v[1]))}_{'fp16' if v[2] else 'fp32'}_{'near' if v[3] else 'nonear'}"
               f"_{v[4]}_pad{v[5]}_x{v[6]:g}" for v in VARIANTS]
