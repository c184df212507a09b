"""Cases, float64 references, bounds and a branch classifier for the per-ray compositing and glue kernels
(csrc/composite.hip: accumulate_kernel, accumulate_bwd_kernel, composite_fwd_kernel, composite_bwd_kernel,
embedding_lerp_*; csrc/train_fused.hip: sdf_render_fwd/bwd_kernel and their _pair forms, prop_weights_*, appearance_*):
tests/test_composite_refs_host.py on the CPU, tests/test_gpu_composite_exact.py on the GPU.

THE BRANCHES.  Every feature loop picks one of three forms from the channel count C and from pointer alignment
(`feature_path`, a restatement of the kernels' own conditions):
  vec4     LP = C / 4 lanes share a sample, 64 / LP samples per pass: C % 4 == 0, LP a power of two <= 64, 16-byte aligned
           pointers (composite_bwd: features, gF, gf; sdf_render_fwd: features and THE RAY'S output row; sdf_render_bwd:
           features, gfeat and THE RAY'S gF row -- with an odd row stride the rays of one launch part ways)
  flat     C <= 64 and 64 % C == 0: a lane always sees the same channel, lanes are xor-reduced down to off >= C
           (accumulate, accumulate_bwd, composite_fwd; the fallback of sdf_render_fwd)
  generic  ch = lane, lane + 64, ... in the forwards, a lane per sample with a serial channel loop in the backwards
`COVER` lists every (path, class) a kernel has; the case tables below are generated and checked against it.
`pair_taken` restates the launchers' choice of the two-rays-per-wave kernels.

THE LATTICE FAMILY: one right answer per element, compared bit for bit.
  features, gF, gD, gA, gWns   small integers;  bin edges integers whose midpoints (e0 + e1) / 2 are integers
  composite / accumulate       the weights are given: 2^-k (k = 1 .. n, each once) at n <= 16 sample indices, among them 0, 63,
                               64, 65, S - 2 and S - 1 where they exist, 0 elsewhere; the last ray of a case with several rays
                               has no weight at all (its sky residual is 1)
  sdf_render, SDF head         sdf in {0, +256, -256}, beta a power of two in [1/2, 4], beta_min = 0.  The kernel forms
                               alpha = 1 / (1 + __expf(sdf beta)):  sdf = 0 -> 1 / (1 + 1) = 1/2;  sdf = +256 -> __expf(>= 128)
                               = inf, 1 / inf = 0;  sdf = -256 -> __expf(<= -128) < 2^-149 is 0, 1 / 1 = 1
                               (`alpha_of_lattice_sdf` does this in numpy fp32 and the host test asserts the three values).
                               At most 8 samples of a ray have alpha = 1/2: every T is 2^-j, every weight 2^-j or 0
  sdf_render, density head     x in {+256, -256}: expf(256) = inf, -expm1f(-inf) = 1;  expf(-256) = 0, -expm1f(-0) = 0: a
                               selector, weights 0 or 1
  prop_weights                 densities in {0, 2^20} on bins of integer length >= 1: a step is 0 or >= 2^20, expf(-step) is 1
                               or 0, the weights are 1 on the first dense bin and 0 elsewhere, whatever the carry's rounding
`assert_exact` proves from a case's own numbers that every sum the kernels form -- sum |w||f|, sum |gF||f|, sum |w||mid|, the
suffix sums sum |gw a T| of the backward -- is, in units of the case's quantum 2^-K, an integer below 2^24.  Every partial
sum of any subset of the terms, in any order and grouping, through fmaf or a separate multiply and add, is then
representable: fp32 has nothing to round, and bit equality does not depend on the path or the shuffle order a kernel uses.
What can NOT be exact here moves to the graded family: d beta (identically 0 in the lattice: the gradient passes only
where sdf = 0), and the density head's d x (times expf(+-15), which rounds).

THE GRADED FAMILY: generic values, float64 reference, per element |got - ref| <= bound with the rounding counts that
tests/test_gpu_saturation.py derives (sharp_refs.check / ref_alpha / ref_density), restated with C in them where that
file fixes C = 32:
  acc 2 S U sum w;  features 2 (S + 4) U (sum |w2||f| + (1 + sum w) |f_last|)  [x2 in sdf_render: the weights round too];
  depth 2 (S + 2) U sum |w||mid|;  d features 2 (S + 2) U (|w2 gF| + (1 + sum w) |gF|);  d weights 2 (C + 4) U (sum |gF||f| +
  the same of the last sample + |gA| + |gD mid|);  d sdf 4 (S + C + 8) U mag(d alpha) alpha (1 - alpha) beta
No bound is fitted to a kernel's output.  The reference composites the kernel's OWN fp32 alphas after holding them to a
float64 sigmoid, as tests/test_gpu_saturation.py does.

DEFECTS (`DEFECTS`): the references take `defect=` and plant one wrong-but-plausible behaviour; the host test shows that
each makes the comparison used on the GPU fail.

APPEARANCE / EMBEDDING: table integers in [-3, 3], duration and n_per powers of two, times multiples of
duration / (8 n_per): t / duration * n_per is a multiple of 1/8, the slot and the fraction are exact, every forward value
a (1 - f) + b f and every backward sum of g (1 - f), g f (|g| <= 3, at most 4097 rays: below 2^24 eighths) is exact in any
atomic order."""
from dataclasses import dataclass

import numpy as np

import synth
from sharp_refs import TINY, U, ref_alpha, ref_density

LIMIT = 2 ** 24
BIG = 256.0  # |sdf| (|x| of the density head) of a saturated lattice sample
DENSE = 2.0 ** 20  # density of a dense bin of the prop_weights lattice
C_ALL = (1, 2, 3, 4, 8, 12, 16, 32, 64, 65, 100, 128, 256, 512)
S_SCAN = (2, 3, 31, 32, 33, 63, 64, 65, 128, 129)
S_PROP = S_SCAN + (193,)  # four chunks: the carry loop of prop_weights_bwd runs three times
S_COMP = (1, 2, 15, 16, 17, 63, 64, 65, 129)
R_ALL = (1, 4, 5, 9)  # one wave; a full workgroup; three idle waves; an odd count (the pair kernels' last upper half)
S_FWD_MAX, S_BWD_MAX = 2048, 1024  # sdf_render's documented limits
ERR_UNSUPPORTED = 2  # NRHIP_ERR_UNSUPPORTED (include/neurad_hip.h)

FLAT_KERNELS = ("accumulate", "accumulate_bwd", "composite_fwd")
VEC4_KERNELS = ("composite_bwd", "sdf_render_fwd", "sdf_render_bwd")
PAIR_KERNELS = ("sdf_render_fwd_pair", "sdf_render_bwd_pair")
KERNELS = FLAT_KERNELS + VEC4_KERNELS + PAIR_KERNELS
DEFECTS = ("sky_on_s_minus_2", "tail_sample_dropped", "channel_group_swapped", "w_ns_includes_last",
           "upper_half_wrong_ray", "carry_lost_at_64")
ALIGNS = ("aligned", "feat_off", "odd_out", "odd_g")


# ---- the branch classifier ---------------------------------------------------------------------------------------------
def vec4_ok(C):
    LP = C >> 2
    return C % 4 == 0 and 1 <= LP <= 64 and (LP & (LP - 1)) == 0


def flat_ok(C):
    return C <= 64 and 64 % C == 0


def feature_path(kernel, C, aligned=True):
    """"vec4" | "flat" | "generic": the inner loop `kernel` takes at C channels; `aligned`: every pointer the kernel's own
    test looks at is on the 16-byte grid (see the module text for which those are)"""
    assert kernel in KERNELS, kernel
    if kernel in PAIR_KERNELS:
        assert C == 32 and aligned  # the launchers send nothing else there
        return "vec4"
    if kernel in VEC4_KERNELS and vec4_ok(C) and aligned:
        return "vec4"
    if kernel in FLAT_KERNELS or kernel == "sdf_render_fwd":
        return "flat" if flat_ok(C) else "generic"
    return "generic"


def pair_taken(S, C, stride, aligned, switch, head="sdf"):
    """the launchers of sdf_render_fwd / _bwd: two rays per wave when NRHIP_SDF_RENDER_PAIR is 1, the SDF head, S <= 32,
    C == 32, the row stride (out_stride / g_stride) a multiple of 4 and the base pointers 16-byte aligned"""
    return bool(switch) and head == "sdf" and S <= 32 and C == 32 and stride % 4 == 0 and bool(aligned)


def branch(kernel, C, aligned=True):
    """(path, class): vec4 by LP, flat by C, generic by why it was taken"""
    path = feature_path(kernel, C, aligned)
    off = kernel in VEC4_KERNELS and vec4_ok(C) and not aligned
    if path == "vec4":
        return path, C >> 2
    if path == "flat":
        return path, "misaligned" if off else C
    return path, "misaligned" if off else ("small" if C < 64 else ("wide" if C >= 512 else "stride"))


_LPS = (1, 2, 4, 8, 16, 32, 64)
_GENERIC = [("generic", k) for k in ("small", "stride", "wide")]  # C < 64; 64 < C < 512: the ch += 64 stride steps; LP = 128
COVER = {
    **{k: [("flat", c) for c in _LPS] + _GENERIC for k in FLAT_KERNELS},
    "composite_bwd": [("vec4", lp) for lp in _LPS] + _GENERIC + [("generic", "misaligned")],
    "sdf_render_fwd": [("vec4", lp) for lp in _LPS] + [("flat", 1), ("flat", 2), ("flat", "misaligned")] + _GENERIC
    + [("generic", "misaligned"), ("mixed", "per ray")],
    "sdf_render_bwd": [("vec4", lp) for lp in _LPS] + _GENERIC + [("generic", "misaligned"), ("mixed", "per ray")],
    "sdf_render_fwd_pair": [("vec4", 8)],
    "sdf_render_bwd_pair": [("vec4", 8)],
}


# which path each width takes with aligned pointers, per kernel (the pair kernels exist at C = 32 only)
WIDTH_PATHS = {k: {C: feature_path(k, C) for C in C_ALL} for k in FLAT_KERNELS + VEC4_KERNELS}


# ---- cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    op: str  # "accumulate" | "composite" | "sdf_render" | "prop_weights"
    R: int
    S: int
    C: int = 1
    align: str = "aligned"  # ALIGNS: features one float off; an odd output stride (extra_cols = 1); gF in a wider odd row
    head: str = "sdf"  # sdf_render: "sdf" | "density"
    es_extra: int = 0  # prop_weights: edge rows wider than S + 1 by this much

    @property
    def id(self):
        tail = "".join(f"-{t}" for t in (self.align != "aligned" and self.align, self.head != "sdf" and self.head,
                                          self.es_extra and f"es+{self.es_extra}") if t)
        return f"R{self.R}-S{self.S}-C{self.C}{tail}"

    @property
    def seed(self):
        return 1000 * self.S + 10 * self.C + self.R


OP_KERNELS = {"accumulate": ("accumulate", "accumulate_bwd"), "composite": ("composite_fwd", "composite_bwd"),
              "sdf_render": ("sdf_render_fwd", "sdf_render_bwd")}


def ray_aligned(case, kernel, r):
    """does ray r of `case` pass `kernel`'s alignment test"""
    if case.align == "aligned" or kernel in FLAT_KERNELS:
        return True
    if case.align == "feat_off":
        return False
    if case.align == "odd_out":
        return kernel != "sdf_render_fwd" or (r * (case.C + 1)) % 4 == 0
    return kernel != "sdf_render_bwd" or (r * (case.C + 1)) % 4 == 0  # odd_g


def case_pair(case, kernel, switch):
    """does the launcher send `case` to `kernel`'s pair form"""
    stride = case.C + 1 if (case.align, kernel) in (("odd_out", "sdf_render_fwd"), ("odd_g", "sdf_render_bwd")) else case.C
    base_ok = case.align != "feat_off"
    return case.op == "sdf_render" and pair_taken(case.S, case.C, stride, base_ok, switch, case.head)


def branches(case, kernel, switch=False):
    """the set of (path, class) that the rays of `case` take in `kernel`; rays that part ways add ("mixed", "per ray")"""
    if case_pair(case, kernel, switch):
        return {branch(kernel + "_pair", case.C)}
    got = {branch(kernel, case.C, ray_aligned(case, kernel, r)) for r in range(case.R)}
    return got | {("mixed", "per ray")} if len(got) > 1 else got


def spw_of(kernel, C, aligned=True):
    """samples per pass of the kernel's feature loop (what `tail_sample_dropped` drops behind)"""
    path = feature_path(kernel, C, aligned)
    return 64 // (C >> 2) if path == "vec4" else (max(1, 64 // C) if path == "flat" else 64)


def _uniq(cases):
    return list(dict.fromkeys(cases))


def _table(op, widths, s_list):
    """every width at a sample count from the list and at an odd one (a tail behind the last full pass of every float4
    width: S % (64 / LP) != 0 for every LP < 64), then every sample count at a narrow width.  C > 64 stays at S <= 65,
    C = 512 at S <= 17."""
    out = []
    for i, C in enumerate(widths):
        ss = [s for s in s_list if s <= (17 if C > 256 else (65 if C > 64 else 10 ** 9))]
        odd = [s for s in ss if s % 2 and s > 1]
        out.append(Case(op, R_ALL[i % 4], ss[(2 * i) % len(ss)], C))
        out.append(Case(op, R_ALL[(i + 1) % 4] if C <= 64 else (1, 4)[i % 2], odd[i % len(odd)], C))
    for j, S in enumerate(s_list):
        out.append(Case(op, R_ALL[(j + 2) % 4], S, (32, 4, 3, 8)[j % 4]))
    return _uniq(out)


# the flat kernels need no 128 / 256 (generic "stride" like 65 and 100); the float4 kernels take every width
ACC_CASES = _table("accumulate", (1, 2, 3, 4, 8, 12, 16, 32, 64, 65, 100, 512), S_COMP)
COMP_CASES = _table("composite", C_ALL, S_COMP) + [Case("composite", 5, 17, 32, "feat_off"),
                                                   Case("composite", 4, 65, 4, "feat_off"),
                                                   Case("composite", 1, 15, 128, "feat_off")]
SDF_LONG = (Case("sdf_render", 2, S_FWD_MAX, 4), Case("sdf_render", 2, S_BWD_MAX, 4))  # forward only / forward and backward
SDF_ALIGN = [Case("sdf_render", R, S, C, a) for a in ALIGNS[1:] for R, S, C in ((5, 17, 32), (9, 33, 4), (4, 31, 32))] + [
    Case("sdf_render", 4, 15, 128, "feat_off"), Case("sdf_render", 5, 3, 256, "odd_out"), Case("sdf_render", 5, 3, 64, "odd_g")]
SDF_PAIR = [Case("sdf_render", R, S, 32) for R, S in ((1, 2), (4, 3), (5, 31), (9, 32), (9, 17), (5, 33))]
SDF_DENSITY = [Case("sdf_render", R, S, C, head="density") for R, S, C in ((5, 17, 32), (4, 65, 4), (9, 129, 3), (1, 32, 32),
                                                                            (4, 64, 64), (5, 33, 100))]
SDF_CASES = _uniq(_table("sdf_render", C_ALL, S_SCAN) + SDF_PAIR + SDF_ALIGN + SDF_DENSITY + list(SDF_LONG))
PROP_CASES = [Case("prop_weights", R_ALL[i % 4], S, es_extra=(0, 3, 0, 1)[i % 4]) for i, S in enumerate(S_PROP)] + [
    Case("prop_weights", 5, 1), Case("prop_weights", 9, 193, es_extra=2)]


def has_backward(case):
    return case.S <= S_BWD_MAX


# ---- exactness ----------------------------------------------------------------------------------------------------------
def quantum(*arrays):
    """the smallest K with every value a multiple of 2^-K"""
    for K in range(0, 64):
        if all(np.array_equal(np.asarray(a, np.float64) * 2.0 ** K, np.rint(np.asarray(a, np.float64) * 2.0 ** K))
               for a in arrays):
            return K
    raise AssertionError("not dyadic")


def _fits(what, mags, K):
    """a sum of magnitudes (already summed), in units of 2^-K: below 2^24"""
    m = float(np.max(mags, initial=0.0)) * 2.0 ** K
    assert m < LIMIT, f"{what}: {m} >= 2^24 in units of 2^-{K}"
    return m


def same(got, want, what):
    """bit equality by value with the float64 reference: nothing unwritten (NaN prefill), nothing different"""
    got = np.asarray(got)
    want = np.broadcast_to(np.asarray(want, np.float64), got.shape)
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} of {got.size} elements unwritten or NaN, first " \
                                    f"{np.argwhere(np.isnan(got))[0].tolist()}"
    bad = got.astype(np.float64) != want
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements differ, first {list(k)}: got {got[k]!r} "
                             f"want {want[k]!r}")


def worst(got, ref, bound):
    """max err / bound over the elements (0 / 0 counts as 0): printed by the graded GPU tests before they assert"""
    got, ref, bound = (np.broadcast_to(np.asarray(v, np.float64), np.shape(got)) for v in (got, ref, bound))
    err = np.where(np.isfinite(ref), np.abs(got - ref), 0.0)
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0), initial=0.0))


# ---- inputs -------------------------------------------------------------------------------------------------------------
def ints(shape, lo, hi, seed):
    return np.clip(np.floor(synth.uniform(shape, lo, hi + 1, seed)), lo, hi).astype(np.float32)


def chosen(S, n, seed, must=True):
    """up to n sample indices of a ray, ascending: 0, 63, 64, 65, S - 2, S - 1 where they exist, the rest drawn"""
    first = sorted({i for i in (0, 63, 64, 65, S - 2, S - 1) if 0 <= i < S}) if must else []
    order = np.argsort(synth.uniform((S,), 0.0, 1.0, seed), kind="stable").tolist()
    return np.array(sorted((first + [i for i in order if i not in first])[:n]), np.int64)


def int_edges(R, S, seed):
    """[R, S + 1] integer edges, steps of 2 or 4 from an even start: every bin has an integer midpoint and length >= 2"""
    step = 2.0 * ints((R, S), 1, 2, seed)
    e0 = 2.0 * ints((R, 1), 0, 5, seed + 1)
    return np.concatenate([e0, e0 + np.cumsum(step, -1)], -1).astype(np.float32)


def lattice_weights(case):
    R, S = case.R, case.S
    w = np.zeros((R, S), np.float64)
    for r in range(R):
        if R > 1 and r == R - 1:
            continue  # the ray without a weight: sky residual 1
        idx = chosen(S, 16, case.seed + r, must=r % 2 == 0)
        k = 1 + np.argsort(synth.uniform((len(idx),), 0.0, 1.0, case.seed + 100 + r), kind="stable")
        w[r, idx] = 2.0 ** -k.astype(np.float64)
    return w.astype(np.float32)


def lattice_inputs(case):
    """the lattice family's inputs of `case`, float32 arrays by name"""
    R, S, C, sd = case.R, case.S, case.C, case.seed
    d = {"f": ints((R, S, C), -4, 4, sd + 1), "gF": ints((R, C), -2, 2, sd + 2), "gD": ints((R, 1), -3, 3, sd + 3),
         "gA": ints((R, 1), -3, 3, sd + 4), "e": int_edges(R, S, sd + 5)}
    if case.op in ("accumulate", "composite"):
        d["w"] = lattice_weights(case)
        m = ints((R, S), 1, 30, sd + 8)  # starts and ends are two tensors here: any integer midpoint, not monotone
        d["st"], d["en"] = m - 1, m + 1
    elif case.op == "sdf_render":
        d["gWns"] = ints((R, S - 1), -3, 3, sd + 6)
        x = np.full((R, S), BIG, np.float32)  # alpha = 0
        for r in range(R):
            kind = r % 4  # 0: halves at the edge indices; 1: halves, then an opaque sample; 2: empty; 3: halves anywhere
            if case.head == "density":
                if kind != 2:
                    x[r, chosen(S, 3, sd + r, must=False)] = -BIG
                continue
            if kind == 2:
                continue
            idx = chosen(S, 8, sd + r, must=kind != 3)
            x[r, idx] = 0.0
            if kind == 1 and len(idx) > 1:
                x[r, idx[len(idx) // 2]] = -BIG
        d["x"] = -x if case.head == "density" else x  # the density head's dense samples are x = +BIG
        d["beta"] = np.array([(1.0, 4.0, 0.5)[case.S % 3]], np.float32)
    else:
        e = int_edges(R, S + case.es_extra, sd + 5)
        d = {"e": e, "gw": ints((R, S), -3, 3, sd + 6), "gd": ints((R, 1), -3, 3, sd + 7),
             "dens": np.zeros((R, S), np.float32)}
        for r in range(R):
            if r % 4 != 2:  # (ray 2: no dense bin at all)
                idx = chosen(S, 4, sd + r, must=False)
                idx = idx[(r % 4 == 1) * (len(idx) // 2):]  # rays 1: the first hit further back
                d["dens"][r, idx] = DENSE
    return d


def graded_inputs(case):
    R, S, C, sd = case.R, case.S, case.C, case.seed + 7
    e = np.cumsum(synth.uniform((R, S + 1 + case.es_extra), 0.05, 0.5, sd), -1).astype(np.float32)
    d = {"f": synth.normal((R, S, C), sd + 1), "gF": synth.normal((R, C), sd + 2), "gD": synth.normal((R, 1), sd + 3),
         "gA": synth.normal((R, 1), sd + 4), "e": e}
    if case.op in ("accumulate", "composite"):
        a = synth.uniform((R, S), 0.02, 0.5, sd + 5).astype(np.float64)
        T = np.cumprod(np.concatenate([np.ones((R, 1)), 1 - a[:, :-1]], -1), -1)
        d["w"] = (a * T).astype(np.float32)
    elif case.op == "sdf_render":
        d["gWns"] = synth.normal((R, S - 1), sd + 6)
        if case.head == "density":
            d["x"] = synth.uniform((R, S), -1.0, 3.0, sd + 7)  # sigma delta in [0.018, 10]
            if S > 3:
                e[:, 3] = e[:, 2]  # one zero-length bin per ray
            e[::2, S] = 1e10  # sky
        else:
            d["x"] = (synth.normal((R, S), sd + 7) * 0.5).astype(np.float32)
            e[::2, S] = 1e10
            d["beta"] = np.array([1.9], np.float32)
            d["beta_min"] = 0.1
    else:
        # total optical depth ~ 3 per ray whatever S: the carry matters in every chunk and the last T is not 0
        d = {"e": e, "gw": synth.normal((R, S), sd + 6), "gd": synth.normal((R, 1), sd + 7),
             "dens": (np.exp(synth.uniform((R, S), -1.5, 1.5, sd + 8)) * np.float32(8.0 / S)).astype(np.float32)}
    return d


def alpha_of_lattice_sdf(sdf, beta):
    """the kernel's sigmoidf_(-sdf beta) = 1 / (1 + __expf(sdf beta)) in numpy fp32"""
    with np.errstate(over="ignore", under="ignore"):
        x = np.float32(-1.0) * np.asarray(sdf, np.float32) * np.float32(beta)
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def lattice_alpha(case, d):
    """the lattice family's alphas, exactly 0, 1/2 or 1"""
    if case.head == "density":
        return (d["x"] > 0).astype(np.float64)
    return alpha_of_lattice_sdf(d["x"], d["beta"][0]).astype(np.float64)


# ---- references ---------------------------------------------------------------------------------------------------------
def _swap_groups(a, r):
    """float4 groups 0 and 1 of ray r exchanged (last axis = channels)"""
    if a.shape[-1] >= 8:
        a[r, ..., 0:4], a[r, ..., 4:8] = a[r, ..., 4:8].copy(), a[r, ..., 0:4].copy()


def mids(e, S):
    return ((e[:, :S] + e[:, 1:S + 1]) / np.float32(2)).astype(np.float64)


def bins(d, S):
    """(starts, ends) of a case's inputs: given as such (composite: two tensors), or the edges' two views"""
    return (d["st"], d["en"]) if "st" in d else (d["e"][:, :S], d["e"][:, 1:S + 1])


def _w_ns_rows_of_s(w_ns, R, S):
    """`w_ns_includes_last`: rows S wide written into a buffer of rows S - 1 wide"""
    flat = np.zeros(R * S)
    flat[(np.arange(R)[:, None] * S + np.arange(S - 1)[None]).ravel()] = w_ns.ravel()
    return flat[:R * (S - 1)].reshape(R, S - 1)


def ref_composite(w32, feats, st, en, defect=None, spw=1):
    """C2 in float64 from the kernel's fp32 weights -> w2 (the sky residual on the last sample), features, depth, acc, mid"""
    w = w32.astype(np.float64)
    S = w.shape[1]
    acc = w.sum(-1, keepdims=True)
    w2 = w.copy()
    w2[:, -2 if (defect == "sky_on_s_minus_2" and S > 1) else -1] += 1 - acc[:, 0]
    f = feats.astype(np.float64)
    wf = w2.copy()
    if defect == "tail_sample_dropped":
        wf[:, (S // spw) * spw:] = 0
    of = (wf[..., None] * f).sum(1)
    if defect == "channel_group_swapped":
        _swap_groups(of, w.shape[0] // 2)
    mid = ((st + en) / np.float32(2)).astype(np.float64)
    return w2, of, (w2[:, :-1] * mid[:, :-1]).sum(-1, keepdims=True), acc, mid


def ref_composite_bwd(w2, feats, mid, gF, gD=None, gA=None, gWns=None, defect=None, spw=1):
    """df_sc = w2_s gF_c;  dw_s = q_s - q_{S-1} + g_acc + (g_depth mid_s + gWns_s) [s < S - 1],  q_s = sum_c gF_c f_sc
    -> d features, d weights, the magnitude sum of d weights' terms"""
    R, S = w2.shape
    f, g = feats.astype(np.float64), gF.astype(np.float64)
    zero = np.zeros((R, 1))
    gD, gA = (zero if v is None else np.asarray(v, np.float64).reshape(R, 1) for v in (gD, gA))
    gf = w2[..., None] * g[:, None, :]
    q, qm = (f * g[:, None, :]).sum(-1), (np.abs(f) * np.abs(g)[:, None, :]).sum(-1)
    dm = np.where(np.arange(S)[None] < S - 1, gD * mid, 0.0)
    gwn = np.zeros((R, S)) if gWns is None else np.concatenate([gWns.astype(np.float64), zero], -1)
    gw = q - q[:, -1:] + gA + dm + gwn
    mag = qm + qm[:, -1:] + np.abs(gA) + np.abs(dm) + np.abs(gwn)
    if defect == "tail_sample_dropped":
        gf[:, (S // spw) * spw:] = 0
        gw[:, (S // spw) * spw:] = 0
    if defect == "channel_group_swapped":
        _swap_groups(gf, R // 2)
    return gf, gw, mag


def ref_accumulate(w32, v32, g32=None, defect=None, spw=1):
    """out[r, c] = sum_s w v (values None: sum_s w);  backward gw = sum_c g v, gv = w g -> out, gw, gv"""
    w = w32.astype(np.float64)
    R, S = w.shape
    if v32 is None:
        return w.sum(-1, keepdims=True), None, None
    v = v32.astype(np.float64)
    wf = w.copy()
    if defect == "tail_sample_dropped":
        wf[:, (S // spw) * spw:] = 0
    out = (wf[..., None] * v).sum(1)
    if defect == "channel_group_swapped":
        _swap_groups(out, R // 2)
    if g32 is None:
        return out, None, None
    g = g32.astype(np.float64)
    gw, gv = (v * g[:, None, :]).sum(-1), wf[..., None] * g[:, None, :]
    if defect == "tail_sample_dropped":
        gw[:, (S // spw) * spw:] = 0
    if defect == "channel_group_swapped":
        _swap_groups(gv, R // 2)
    return out, gw, gv


def _chunks(S):
    return [slice(s0, min(s0 + 64, S)) for s0 in range(0, S, 64)]


def _excl_prod(a):
    return np.cumprod(np.concatenate([np.ones_like(a[:, :1]), 1 - a[:, :-1]], -1), -1)


def _suffix_excl(v):
    return np.concatenate([np.flip(np.cumsum(np.flip(v[:, 1:], -1), -1), -1), np.zeros_like(v[:, :1])], -1)


def _trans(a, defect=None):
    """exclusive product of 1 - alpha; `carry_lost_at_64`: every 64-sample pass starts again from 1"""
    if defect != "carry_lost_at_64":
        return _excl_prod(a)
    return np.concatenate([_excl_prod(a[:, c]) for c in _chunks(a.shape[1])], -1)


def _pair_defect(outs, defect):
    if defect == "upper_half_wrong_ray":
        for k, v in outs.items():
            if v is not None and np.ndim(v) >= 1 and np.shape(v)[0] > 1:
                v[1::2] = v[0::2][: len(v[1::2])]
    return outs


def lattice_sdf_render(case, d, defect=None):
    """the lattice family's one right answer of sdf_render_fwd and _bwd, float64, by the kernels' own formulas:
    T = exclusive product, w = alpha T, the sky residual on the last sample, ga_i = gw_i T_i - (sum_{k>i} gw_k a_k T_k) /
    (1 - a_i) (not formed where a_i = 1: the factor a (1 - a) is 0 there), d sdf = -ga a (1 - a) beta"""
    R, S, C = case.R, case.S, case.C
    a = lattice_alpha(case, d)
    T = _trans(a, defect)
    w = a * T
    spw_f, spw_b = spw_of("sdf_render_fwd", C), spw_of("sdf_render_bwd", C)
    e = d["e"]
    mid = mids(e, S)
    w2, of, depth, acc, _ = ref_composite(w.astype(np.float32), d["f"], e[:, :S], e[:, 1:S + 1], defect, spw_f)
    w_ns = w[:, :-1].copy()
    if defect == "w_ns_includes_last":
        w_ns = _w_ns_rows_of_s(w_ns, R, S)
    out = {"alpha": a, "w_ns": w_ns, "out": of, "depth": depth, "acc": acc}
    if has_backward(case):
        gf, gw, _ = ref_composite_bwd(w2, d["f"], mid, d["gF"], d["gD"], d["gA"], d["gWns"], defect, spw_b)
        term = gw * a * T
        after = _suffix_excl(term)
        if defect == "carry_lost_at_64":  # the suffix of the later passes lost as well
            after = np.concatenate([_suffix_excl(term[:, c]) for c in _chunks(S)], -1)
        out["gfeat"] = gf
        if case.head == "sdf":
            ga = gw * T - np.where(a == 1, 0.0, after / np.where(a == 1, 1.0, 1 - a))
            out["gsdf"] = -(ga * a * (1 - a)) * float(d["beta"][0])
            out["gbeta"] = np.zeros(1)
    return _pair_defect(out, defect)


def assert_exact(case, d):
    """the lattice case's sums fit: -> the largest sum, in units of the case's quantum (see the module text)"""
    S = case.S
    top = 0.0
    if case.op == "prop_weights":
        e = d["e"].astype(np.float64)
        delta, mid = e[:, 1:S + 1] - e[:, :S], mids(d["e"], S)
        assert quantum(e, mid, d["gw"], d["gd"]) == 0 and (delta >= 1).all()
        assert np.isin(d["dens"], (0.0, DENSE)).all()
        G = np.abs(d["gw"].astype(np.float64)) + np.abs(d["gd"].astype(np.float64)) * mid
        # one weight of 1 per ray: depth = its midpoint; d dens_i = (G_i - G_hit) delta_i in front of the hit, 0 behind
        return max(_fits("depth", mid, 0), _fits("d dens", 2 * G.max(-1, keepdims=True) * delta, 0))
    f, gF = np.abs(d["f"].astype(np.float64)), np.abs(d["gF"].astype(np.float64))
    st, en = bins(d, S)
    mid = ((st + en) / np.float32(2)).astype(np.float64)
    if case.op == "sdf_render":
        a = lattice_alpha(case, d)
        assert np.isin(a, (0.0, 0.5, 1.0)).all()
        T = _trans(a)
        w = a * T
    else:
        w = d["w"].astype(np.float64)
    acc = w.sum(-1, keepdims=True)
    w2 = np.abs(w).copy()
    w2[:, -1] += np.abs(1 - acc[:, 0])
    K = quantum(w, 1 - acc, *((T,) if case.op == "sdf_render" else ()))
    assert quantum(f, gF, mid, d["gD"], d["gA"], st, en) == 0
    top = max(top, _fits("acc and the residual", 1 + 2 * np.abs(w).sum(-1), K))
    top = max(top, _fits("features", (w2[..., None] * f).sum(1), K))
    top = max(top, _fits("depth", (np.abs(w) * mid).sum(-1), K))
    top = max(top, _fits("d features", w2[..., None] * gF[:, None, :], K))
    gwm = (f * gF[:, None, :]).sum(-1)
    gwm = gwm + gwm[:, -1:] + np.abs(d["gA"]) + np.abs(d["gD"]) * mid
    if case.op == "sdf_render":
        gwm[:, :-1] += np.abs(d["gWns"])
    top = max(top, _fits("d weights", gwm, 0))
    if case.op == "accumulate":
        top = max(top, _fits("gv", np.abs(w)[..., None] * gF[:, None, :], K))
    if case.op == "sdf_render" and case.head == "sdf" and has_backward(case):
        term = gwm * a * T  # multiples of 2^-(K + 1)
        suffix = term.sum(-1, keepdims=True)
        top = max(top, _fits("suffix sums", suffix, K + 1))
        # ga = gw T - after / (1 - a): 1 - a is 1 or 1/2; ds = ga / 4; d sdf = ds beta, beta a power of two
        top = max(top, _fits("d alpha", gwm * T + 2 * suffix, K + 1))
        b = float(d["beta"][0])
        assert b in (0.5, 1.0, 2.0, 4.0) and (np.abs(d["x"]) * b >= 128)[d["x"] != 0].all()
    return top


# ---- the graded family's references and bounds ---------------------------------------------------------------------------
def graded_composite(case, d, defect=None):
    """-> {name: (reference, bound)} of composite_fwd and composite_bwd; the counts of tests/test_gpu_saturation.py"""
    S, C = case.S, case.C
    st, en = bins(d, S)
    w2, rf, rd, ra, mid = ref_composite(d["w"], d["f"], st, en, defect, spw_of("composite_fwd", C))
    sw = d["w"].astype(np.float64).sum(-1, keepdims=True)
    absf = np.abs(d["f"].astype(np.float64))
    gF64 = d["gF"].astype(np.float64)
    out = {"acc": (ra, 2 * S * U * sw),
           "features": (rf, 2 * (S + 4) * U * ((np.abs(w2)[..., None] * absf).sum(1) + (1 + sw) * absf[:, -1])),
           "depth": (rd, 2 * (S + 2) * U * (np.abs(w2[:, :-1]) * np.abs(mid[:, :-1])).sum(-1, keepdims=True))}
    rgf, rgw, mag = ref_composite_bwd(w2, d["f"], mid, d["gF"], d["gD"], d["gA"], None, defect, spw_of("composite_bwd", C))
    out["d features"] = (rgf, 2 * (S + 2) * U * (np.abs(rgf) + (1 + sw)[..., None] * np.abs(gF64)[:, None, :]))
    out["d weights"] = (rgw, 2 * (C + 4) * U * mag)
    return out


def graded_accumulate(case, d, defect=None):
    """out: a chain of at most S fmas and 6 adds; gw: C products; gv: one product"""
    S, C = case.S, case.C
    out, gw, gv = ref_accumulate(d["w"], d["f"], d["gF"], defect, spw_of("accumulate", C))
    w, v, g = (np.abs(d[k].astype(np.float64)) for k in ("w", "f", "gF"))
    return {"out": (out, 2 * (S + 4) * U * (w[..., None] * v).sum(1)),
            "sum w": (d["w"].astype(np.float64).sum(-1, keepdims=True), 2 * (S + 4) * U * w.sum(-1, keepdims=True)),
            "d weights": (gw, 2 * (C + 4) * U * (v * g[:, None, :]).sum(-1)), "d values": (gv, 2 * U * np.abs(gv))}


def graded_alpha(case, d):
    """the float64 alpha of the head and the bound its fp32 form is held to (tests/test_gpu_saturation.py)"""
    S = case.S
    if case.head == "density":
        delta = (d["e"][:, 1:S + 1] - d["e"][:, :S]).astype(np.float64)
        sd = np.exp(d["x"].astype(np.float64)) * delta
        ra = -np.expm1(-sd)
        return ra, TINY + 4 * U * ra + (1 - ra) * 3 * U * sd
    b32 = np.float32(np.abs(d["beta"][0])) + np.float32(d["beta_min"])  # as the kernel forms it
    x = -d["x"].astype(np.float64) * np.float64(b32)
    sig = 1 / (1 + np.exp(-x))
    return sig, TINY + 4 * U * sig + sig * (1 - sig) * 3 * np.abs(x) * U


def graded_sdf_render(case, d, a32, defect=None):
    """-> {name: (reference, bound)} from the kernel's own fp32 alphas `a32` (held to `graded_alpha` by the caller)"""
    R, S, C = case.R, case.S, case.C
    e = d["e"]
    zero = np.zeros((R, S))
    rw, _, _, _ = ref_alpha(a32.astype(np.float32), zero, zero)
    if defect == "carry_lost_at_64":
        rw = a32.astype(np.float64) * _trans(a32.astype(np.float64), defect)
    w2, rf, rd, _, mid = ref_composite(rw, d["f"], e[:, :S], e[:, 1:S + 1], defect, spw_of("sdf_render_fwd", C))
    sw = rw.sum(-1, keepdims=True)
    absf = np.abs(d["f"].astype(np.float64))
    w_ns = _w_ns_rows_of_s(rw[:, :-1], R, S) if defect == "w_ns_includes_last" else rw[:, :-1]
    out = {"w_ns": (w_ns, TINY + 2 * (S + 2) * U * rw[:, :-1]), "acc": (sw, TINY + 2 * (S + 2) * U * sw),
           "out": (rf, 4 * (S + 4) * U * ((np.abs(w2)[..., None] * absf).sum(1) + (1 + sw) * absf[:, -1])),
           "depth": (rd, TINY + 4 * (S + 4) * U * (rw[:, :-1] * np.abs(mid[:, :-1])).sum(-1, keepdims=True))}
    if not has_backward(case):
        return out
    gF64 = d["gF"].astype(np.float64)
    rgf, gw, gw_mag = ref_composite_bwd(w2, d["f"], mid, d["gF"], d["gD"], d["gA"], d["gWns"], defect,
                                        spw_of("sdf_render_bwd", C))
    out["gfeat"] = (rgf, 4 * (S + 4) * U * (np.abs(rgf) + (1 + sw)[..., None] * np.abs(gF64)[:, None, :]))
    _, _, rga, _ = ref_alpha(a32.astype(np.float32), gw, zero)
    _, _, _, mag = ref_alpha(a32.astype(np.float32), gw_mag, zero)
    a64 = a32.astype(np.float64)
    base = 2.0 ** -100 * gw_mag.max(-1, keepdims=True) + 4 * (S + C + 8) * U * mag
    if case.head == "density":
        # alpha = 1 - exp(-e^x delta): d alpha / dx = (1 - alpha) sigma delta, with trunc_exp's exp(clamp(x, -15, 15))
        delta = (e[:, 1:S + 1] - e[:, :S]).astype(np.float64)
        chain = (1 - a64) * delta * np.exp(np.clip(d["x"].astype(np.float64), -15, 15))
        out["gsdf"] = (rga * chain, base * chain)
        return out
    b = float(np.float32(np.abs(d["beta"][0])) + np.float32(d["beta_min"]))
    ds = a64 * (1 - a64)
    bound = base * ds * b
    out["gsdf"] = (-rga * ds * b, bound)
    sdf = d["x"].astype(np.float64)
    out["gbeta"] = (np.array([(rga * ds * -sdf).sum()]),
                    np.array([(bound / b * np.abs(sdf)).sum() + 2 * R * S * U * np.abs(rga * ds * sdf).sum() + 1e-30]))
    return out


def ref_prop_weights(case, d, use_gw=True, use_gd=True, defect=None):
    """-> {name: (reference, bound)} of prop_weights_fwd / _bwd as tests/test_gpu_saturation.py derives them; the upstream
    of each weight is gw + g_depth mid"""
    S = case.S
    e = d["e"]
    delta = e[:, 1:S + 1] - e[:, :S]  # fp32, as the kernel forms it
    mid = mids(e, S)
    zero = np.zeros((case.R, S))
    gw = d["gw"].astype(np.float64) if use_gw else zero
    gd = d["gd"].astype(np.float64) if use_gd else np.zeros((case.R, 1))
    dens = d["dens"]
    rw, _, _, _, fscale, _ = ref_density(delta, dens, gw)
    if defect == "carry_lost_at_64":
        sdl = dens.astype(np.float64) * delta.astype(np.float64)
        cex = np.concatenate([np.concatenate([np.zeros((case.R, 1)), np.cumsum(sdl[:, s0:s0 + 64], -1)[:, :-1]], -1)
                              for s0 in range(0, S, 64)], -1)
        rw = -np.expm1(-sdl) * np.exp(-cex)
    out = {"weights": (rw, TINY + fscale),
           "depth": ((rw * mid).sum(-1, keepdims=True),
                     TINY + ((fscale + S * U * rw) * np.abs(mid)).sum(-1, keepdims=True))}
    G = gw + gd * mid
    _, _, _, rgs, _, gscale = ref_density(delta, dens, G)
    _, _, _, _, _, gscale2 = ref_density(delta, dens, np.abs(gw) + np.abs(gd * mid))
    atol = TINY * (delta.astype(np.float64) + 1) * np.abs(G).max(-1, keepdims=True)
    out["d dens"] = (rgs, atol + gscale + gscale2)
    return out


def lattice_prop_weights(case, d, use_gw=True, use_gd=True, defect=None):
    """the selector: weight 1 on the first dense bin; d dens_i = (G_i - G_hit) delta_i in front of it, 0 from it on"""
    R, S = case.R, case.S
    e = d["e"].astype(np.float64)
    delta, mid = e[:, 1:S + 1] - e[:, :S], mids(d["e"], S)
    dense = d["dens"] > 0
    if defect == "carry_lost_at_64":
        first = np.concatenate([(np.cumsum(dense[:, s0:s0 + 64], -1) == 1) & dense[:, s0:s0 + 64] for s0 in range(0, S, 64)], -1)
    else:
        first = (np.cumsum(dense, -1) == 1) & dense
    w = first.astype(np.float64)
    G = (d["gw"].astype(np.float64) if use_gw else 0.0) + (d["gd"].astype(np.float64) if use_gd else 0.0) * mid
    front = np.cumsum(dense, -1) == 0
    ghit = (G * w).sum(-1, keepdims=True)
    return {"weights": w, "depth": (w * mid).sum(-1, keepdims=True), "d dens": np.where(front, (G - ghit) * delta, 0.0)}


# ---- appearance / embedding ----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class EmbedCase:
    name: str
    R: int
    D: int
    n_sensors: int
    n_per: int
    E: int  # table rows (n_embed); the LDS image holds E * D <= 8192 floats
    temporal: bool = True
    times: bool = True
    bad_sensors: bool = False  # sensor indices -1 and n_sensors among the rays: the clamp
    duration: float = 4.0

    @property
    def in_lds(self):
        return self.E * self.D <= 8192


EMBED_LDS = 8192
GRID_CAP = 256 * 4096  # R * D past which the backward's 256 workgroups take a second grid-stride step
EMBED_CASES = (
    EmbedCase("small", 37, 16, 2, 4, 8),
    EmbedCase("lds-boundary", 41, 256, 4, 8, 32),  # E * D == 8192: the LDS image
    EmbedCase("one-row-over", 41, 256, 4, 8, 33),  # E * D == 8192 + D: global atomics
    EmbedCase("grid-stride-lds", GRID_CAP // 256 + 1, 256, 4, 8, 32),  # R * D == 256 * 4096 + D
    EmbedCase("grid-stride-global", GRID_CAP // 256 + 1, 256, 4, 8, 33),
    EmbedCase("clamp", 29, 16, 2, 4, 8, bad_sensors=True),
    EmbedCase("clamp-global", 29, 256, 4, 8, 33, bad_sensors=True),
    EmbedCase("per-sensor", 33, 16, 3, 1, 3, temporal=False),
    EmbedCase("temporal-without-times", 33, 16, 2, 4, 8, times=False),
)
SENTINEL = np.float32(2.0 ** 40)  # the rows around the table in the larger buffer; exact, and no table value reaches it


def embed_inputs(c):
    R, sd = c.R, 31 * c.R + c.E
    table = ints((c.E, c.D), -3, 3, sd)
    sensor = ints((R,), 0, c.n_sensors - 1, sd + 1).astype(np.int64)
    if c.bad_sensors:
        sensor[::5] = -1
        sensor[2::7] = c.n_sensors
    eighths = ints((R,), 0, 8 * c.n_per, sd + 2)
    eighths[:3] = (0, 8 * c.n_per, 8 * c.n_per - 1)  # t = 0, t = duration, the last slot
    times = (eighths * np.float32(c.duration / (8 * c.n_per))).astype(np.float32)
    return {"table": table, "sensor": sensor, "times": times if c.times else None, "g": ints((R, c.D), -3, 3, sd + 3)}


def embed_slots(c, d, clamp=True):
    """(lo, hi, frac) per ray: the kernels' appearance_slot, clamped into the table as the kernels do (clamp = False: as
    the slot arithmetic leaves them, for embedding_lerp to clamp)"""
    sensor = d["sensor"]
    into = (lambda i: np.clip(i, 0, c.E - 1)) if clamp else (lambda i: i)
    if not (c.temporal and c.times):
        return into(sensor), into(sensor), np.zeros(c.R)
    ti = d["times"].astype(np.float64) / c.duration * c.n_per
    assert np.array_equal(ti * 8, np.rint(ti * 8))
    lo = np.clip(np.floor(ti), 0, c.n_per - 1)
    hi = np.clip(lo + 1, 0, c.n_per - 1)
    return into(lo.astype(np.int64) + sensor * c.n_per), into(hi.astype(np.int64) + sensor * c.n_per), ti - lo


def ref_embed(c, d):
    """-> forward rows [R, D], backward table gradient [E, D]; float64, exact"""
    lo, hi, frac = embed_slots(c, d)
    t = d["table"].astype(np.float64)
    fwd = t[lo] * (1 - frac)[:, None] + t[hi] * frac[:, None] if (c.temporal and c.times) else t[lo]
    g = d["g"].astype(np.float64)
    m = np.zeros((c.E, c.R))  # gw = m g: the slot weights of every ray, summed in float64 (exact: eighths)
    rays = np.arange(c.R)
    np.add.at(m, (lo, rays), 1 - frac)
    np.add.at(m, (hi, rays), frac)
    gw = m @ g
    assert np.abs(g).sum(0).max() * 8 < LIMIT  # every sum of eighths fits
    return fwd, gw


# ---- one entry per op ----------------------------------------------------------------------------------------------------
CASES = {"accumulate": ACC_CASES, "composite": COMP_CASES, "sdf_render": SDF_CASES, "prop_weights": PROP_CASES}
DEFECT_OPS = {"sky_on_s_minus_2": ("composite", "sdf_render"), "tail_sample_dropped": ("accumulate", "composite", "sdf_render"),
              "channel_group_swapped": ("accumulate", "composite", "sdf_render"), "w_ns_includes_last": ("sdf_render",),
              "upper_half_wrong_ray": ("sdf_render",), "carry_lost_at_64": ("sdf_render", "prop_weights")}


def lattice_ref(case, d, defect=None):
    """{name: the one right answer} of the lattice case: the float64 formulas on operands that leave nothing to round"""
    if case.op == "sdf_render":
        return lattice_sdf_render(case, d, defect)
    if case.op == "prop_weights":
        return lattice_prop_weights(case, d, defect=defect)
    ref = (graded_accumulate if case.op == "accumulate" else graded_composite)(case, d, defect)
    return {k: v[0] for k, v in ref.items()}
