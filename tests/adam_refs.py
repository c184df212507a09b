"""References and case builders of the optimizer kernels (csrc/adam.hip): adam_kernel, adam_many_kernel,
adam_prepare_kernel + adam_many_dev_kernel and nonfinite_check_kernel.  tests/test_adam_refs_host.py checks this module on
the CPU, tests/test_gpu_adam_exact.py compares the kernels with it.  Everything here is numpy.

WHAT IS EXACT AND WHY.  The library is built without floating-point contraction, so `adam_elem` is a fixed chain of
correctly rounded fp32 operations (IEEE multiply, add, subtract, divide and square root, two explicit fused multiply-adds,
denormals kept).  `replay` performs the same chain in np.float32 -- numpy's fp32 +, -, *, / and sqrt are correctly rounded,
`fma32` rounds the exact a * b + c once -- so the kernels must give `replay`'s bits, sign of zero included; only a NaN may
differ in its payload (`mismatches`).  The eight scalars of AdamArgs are formed in fp64 and rounded once (`adam_args`);
the host's pow, numpy's and the device's may differ in the last bits of the fp64 value, so the case lists only use
(step, hyper-parameter) combinations whose fp32 roundings survive a relative 2^-48 either way (`robust`).

THE DEAD RULE.  An element with g = m = v = 0 is left alone (p, m, v) when decay == 1 and eps > 0 in fp32: `replay` writes
that out per element, and with eps > 0 the plain arithmetic gives the same bits (m and v become +0 again, m / eps = 0,
p * 1 - step_size * 0 = p with its sign), which the host test proves over the planted values.  m = -0 and v = -0 are outside
the domain: both moments start at +0 and neither update can produce -0.  With eps rounding to 0 the arithmetic gives
0 / 0 = NaN and there is no shortcut.  The fp16 image is the one place where the kernel's GROUP of four shows: a skipped
group (all four elements dead, inside the 16-byte body) keeps its old image, every other element receives half(p_new).

THE ONE BOUND: replay against textbook Adam in fp64 (`adam64`, the formula in the header of adam.hip).  u = 2^-24,
gamma(k) = k u / (1 - k u), every computed scalar of AdamArgs is its fp64 value times (1 + d), |d| <= u, and every fp32
operation below multiplies its exact result by such a factor as long as the result is zero or in fp32's normal range.
  gs   = g * grad_scale                     2 factors (the scalar, the product)
  m'   = fma(gs - m, omb1, m)               CAN cancel, so absolutely: gs's 2, the difference 1, omb1 1, the fma 1 act on terms
                                            of at most M := |m| + (|gs| + |m|) * omb1 in sum: |m'_replay - m'| <= gamma(5) * M
  v'   = fma(b2, v, (omb2 * gs) * gs)       all terms >= 0, no cancellation: omb2 1, gs twice 4, two products 2 (the b2 * v
                                            term has 1), the fma 1: v'_replay = v' (1 + theta_8)
  den  = sqrt(v') * inv + eps               the root halves theta_8 to theta_4 and adds 1, inv 1, the product 1; eps 1; both terms
                                            >= 0; the sum 1: den_replay = den (1 + theta_8)
  U    = step_size * (m' / den)             the quotient 1, step_size 1, the product 1, den's 8: with the exact m',
                                            U (1 + theta_11); m's absolute error passes through |step_size / den| (1 + gamma(11))
  p'   = p * decay - U                      decay 1, the product 1: 2 u |p decay|; the subtraction: u |p'_replay|
Hence, with everything on the right evaluated in fp64,
  |p'_replay - p'| <= (gamma(11) |U| + gamma(5) M |step_size / den| (1 + gamma(11)) + 2 u |p decay|) (1 + u) + u |p'|.
`bound64` returns this where p' is finite in fp64 and every intermediate named above is zero or inside fp32's normal range
with a factor 2 to spare, and inf elsewhere (g = inf / NaN, g^2 under- or overflowing, p = 1e30 ...): there the host test
compares by class (finite, +inf, -inf, NaN where fp64 itself overflows or is undefined) or leaves the element to the
bit-exact GPU comparison, and it asserts that most elements are inside."""
import functools
import math
from collections import namedtuple

import numpy as np

f32, f64, f16 = np.float32, np.float64, np.float16
U = 2.0 ** -24

Args = namedtuple("Args", "step_size b2 omb1 omb2 inv_bc2_sqrt eps decay grad_scale")
Hyper = namedtuple("Hyper", "lr b1 b2 eps wd grad_scale", defaults=(1e-2, 0.9, 0.999, 1e-15, 0.0, 1.0))


# ---- the eight scalars ---------------------------------------------------------------------------------------------------
def adam_args64(step, lr, b1, b2, eps, wd, grad_scale):
    """the fp64 values `make_args` (host) and `adam_prepare_kernel` (device) form before the one rounding"""
    step = float(step)
    with np.errstate(all="ignore"):
        bc1, bc2 = f64(1.0) - f64(b1) ** f64(step), f64(1.0) - f64(b2) ** f64(step)
        return Args(f64(lr) / bc1, f64(b2), f64(1.0 - b1), f64(1.0 - b2), f64(1.0) / np.sqrt(bc2), f64(eps),
                    f64(1.0 - lr * wd), f64(grad_scale))


def adam_args(step, lr, b1, b2, eps, wd, grad_scale):
    with np.errstate(all="ignore"):
        return Args(*[f32(x) for x in adam_args64(step, lr, b1, b2, eps, wd, grad_scale)])


def robust(step, lr, b1, b2, eps, wd, grad_scale):
    """every fp64 scalar, moved by a relative 2^-48 either way, still rounds to the same fp32"""
    for x in adam_args64(step, lr, b1, b2, eps, wd, grad_scale):
        x = float(x)
        if not (f32(x * (1 + 2.0 ** -48)) == f32(x) == f32(x * (1 - 2.0 ** -48))):
            return False
    return True


# ---- exact fp32 arithmetic -----------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """round_fp32(a * b + c), one rounding.  The fp64 product of two fp32 numbers is exact (48 bits).  The fp64 sum s of the
    product and c is rounded; TwoSum gives its error e exactly, and when e != 0 the sum is replaced by round-to-odd (of the
    two fp64 neighbours of the exact value, the one with an odd significand): rounding a round-to-odd fp64 to fp32 (53 >= 24 + 2
    bits) equals rounding the exact value."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(all="ignore"):
        p = a.astype(f64) * b.astype(f64)
        c = c.astype(f64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(f32)


def half_rn(x):
    """fp32 -> fp16, round to nearest even (numpy's conversion)"""
    with np.errstate(all="ignore"):
        return np.asarray(x, f32).astype(f16)


def half_trunc(x):
    """fp32 -> fp16 toward zero (a wrong variant)"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, f32)
        h = x.astype(f16)
        over = np.abs(h.astype(f32)) > np.abs(x)
        return np.where(over & np.isfinite(x), np.nextafter(h, f16(0)), h).astype(f16)


# ---- the kernel's arithmetic ---------------------------------------------------------------------------------------------
def replay(p, g, m, v, args, image=None, *, plain=False, variant=None):
    """adam_elem, operation for operation, on fp32 arrays p, m, v and an fp32 or fp16 gradient; -> (p', m', v', image' or
    None).  image: the fp16 image BEFORE the call, or None.  plain=True: the arithmetic alone, without the dead rule.
    variant: one plausible mistake (VARIANTS that live in the element arithmetic)."""
    a = args
    p, m, v = np.asarray(p, f32), np.asarray(m, f32), np.asarray(v, f32)
    with np.errstate(all="ignore"):
        g32 = np.asarray(g).astype(f32)  # (fp16 -> fp32 is exact)
        if variant == "half_swap" and np.asarray(g).dtype == f16:
            n2 = g32.size // 4 * 4  # lanes of a pair swapped, in the 16-byte body only
            g32 = np.concatenate([g32[:n2].reshape(-1, 2)[:, ::-1].reshape(-1), g32[n2:]])
        gs = g32 * a.grad_scale
        m1 = fma32((g32 if variant == "scale_after_m" else gs) - m, a.omb1, m)
        v1 = fma32(a.b2, v, (a.omb2 * gs) * gs)
        denom = np.sqrt(v1) * a.inv_bc2_sqrt + a.eps
        p1 = p * a.decay - a.step_size * (m1 / denom)
        dead = (g32 == 0) & (m == 0) & (v == 0)
        can_skip = (a.decay == f32(1) or variant == "dead_no_decay") and a.eps > f32(0)
        if not plain and can_skip:
            p1, m1, v1 = np.where(dead, p, p1), np.where(dead, m, m1), np.where(dead, v, v1)
        img = None
        if image is not None:
            img = half_trunc(p1) if variant == "image_trunc" else half_rn(p1)
            if not plain and can_skip:
                n4 = p.size // 4 * 4
                skipped = np.zeros(p.size, bool)
                skipped[:n4] = np.repeat(dead[:n4].reshape(-1, 4).all(-1), 4)
                img = np.where(skipped, np.asarray(image, f16), img)
    return p1.astype(f32), m1.astype(f32), v1.astype(f32), img


def adam64(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale):
    """textbook Adam / AdamW in fp64 from the same fp32 (fp16) inputs -> (p', m', v')"""
    with np.errstate(all="ignore"):
        p, g, m, v = (np.asarray(x).astype(f64) for x in (p, g, m, v))
        g = g * grad_scale
        m1 = m + (g - m) * (1 - b1)
        v1 = b2 * v + (1 - b2) * g * g
        p1 = p * (1 - lr * wd) - (lr / (1 - b1 ** step)) * m1 / (np.sqrt(v1) / math.sqrt(1 - b2 ** step) + eps)
    return p1, m1, v1


def bound64(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale):
    """the bound of the module docstring on |replay - adam64| per element of p'; inf where it does not apply"""
    a = adam_args64(step, lr, b1, b2, eps, wd, grad_scale)
    with np.errstate(all="ignore"):
        p, g, m, v = (np.asarray(x).astype(f64) for x in (p, g, m, v))
        p1, m1, v1 = adam64(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale)
        gs = g * grad_scale
        root = np.sqrt(v1) * float(a.inv_bc2_sqrt)
        den = root + eps
        gam = lambda k: k * U / (1 - k * U)  # noqa: E731
        upd = np.abs(float(a.step_size) * m1 / den)
        M = np.abs(m) + (np.abs(gs) + np.abs(m)) * (1 - b1)
        pd = np.abs(p * float(a.decay))
        bound = (gam(11) * upd + gam(5) * M * np.abs(float(a.step_size) / den) * (1 + gam(11)) + 2 * U * pd) * (1 + U) + U * np.abs(p1)
        lo, hi = 2.0 ** -125, 1.7e38
        normal = lambda x: (x == 0) | ((np.abs(x) >= lo) & (np.abs(x) <= hi))  # noqa: E731
        ok = np.isfinite(p1) & (den > 0)
        for x in (gs, gs - m, (gs - m) * (1 - b1), m1, (1 - b2) * gs, (1 - b2) * gs * gs, b2 * v, v1, root, den, m1 / den, upd, pd, p1):
            ok &= normal(x)
        # an m' that cancels to (nearly) nothing may be denormal in fp32 while its fp64 value is normal, and the other way round
        ok &= (np.abs(m1) >= gam(5) * M + lo) | (m1 == 0)
    return np.where(ok, bound, np.inf)


def mismatches(got, want):
    """indices where two arrays of one dtype differ bit for bit; a NaN matches a NaN of any payload"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    differ = got.view(bits) != want.view(bits)
    if got.dtype.kind == "f":
        differ &= ~(np.isnan(got) & np.isnan(want))
    return np.flatnonzero(differ)


# ---- the launch plan -----------------------------------------------------------------------------------------------------
K_MANY = 24  # descriptors per launch (kAdamMany, kCheckMany)
CAP_ALONE, CAP_SHARED = 4096, 1024

Plan = namedtuple("Plan", "launch blocks passes_first passes_last unrolled_first unrolled_last rem_first rem_last rem2_lanes tail")


def blocks_for(n):
    return int(min(max(((n >> 2) + 255) // 256, 1), CAP_ALONE))


def _passes(first, n_groups, stride):
    return 0 if first >= n_groups else (n_groups - first + stride - 1) // stride


def _check_iters(first, n16, stride):
    i, unrolled, rem = first, 0, 0
    while i + 3 * stride < n16:
        i, unrolled = i + 4 * stride, unrolled + 1
    while i < n16:
        i, rem = i + stride, rem + 1
    return unrolled, rem


def launch_plan(ns, check_half=None, single=False):
    """csrc/adam.hip's launch arithmetic restated.  ns: the element counts of a call's tensors in order (0 = empty).
    single: nrhip_adam_step (one tensor, one launch).  check_half: None for the Adam kernels, else one bool per tensor
    (fp16?) for nonfinite_check_kernel, whose loads are 16 bytes = 4 fp32 or 8 fp16 elements.
    -> (plans, launches): plans[k] is None for an empty tensor, else a Plan: launch index, workgroups, grid-stride passes
    of the first and of the last lane; for the check kernel the unrolled and remainder iterations of the first and last lane,
    how many lanes run the largest remainder count, and the tail length.  launches[j] = indices of the tensors launch j
    holds (a would-be launch that holds none does not happen and is not listed)."""
    ns = [int(n) for n in ns]
    plans, launches = [None] * len(ns), []
    if single:
        assert len(ns) == 1
    k = 0
    while k < len(ns):
        live, j = 0, k
        while j < len(ns) and live < K_MANY:
            live, j = live + (ns[j] > 0), j + 1
        held = []
        while k < len(ns) and len(held) < K_MANY:
            if ns[k] > 0:
                held.append(k)
            k += 1
        if not held:
            continue
        for t in held:
            half = bool(check_half[t]) if check_half is not None else False
            b = blocks_for(ns[t] >> 1 if half else ns[t])
            if b > CAP_SHARED and live > 1 and not single:
                b = CAP_SHARED
            stride = b * 256
            per = 8 if half else 4
            groups = ns[t] // per
            if check_half is None:
                plans[t] = Plan(len(launches), b, _passes(0, groups, stride), _passes(stride - 1, groups, stride),
                                None, None, None, None, None, ns[t] - groups * per)
            else:
                u0, r0 = _check_iters(0, groups, stride)
                u1, r1 = _check_iters(stride - 1, groups, stride)
                # lanes 0 .. x-1 run r0 remainder iterations, the others r0 - 1 (or all of them r0)
                rem2 = stride if r1 == r0 else next(f for f in range(stride) if _check_iters(f, groups, stride)[1] < r0)
                plans[t] = Plan(len(launches), b, None, None, u0, u1, r0, r1, rem2, ns[t] - groups * per)
        launches.append(held)
    return plans, launches


# ---- values --------------------------------------------------------------------------------------------------------------
DENORMAL32 = float(np.float32(2.0 ** -140))
G32_SPECIAL = (0.0, -0.0, DENORMAL32, -DENORMAL32, 1e-20, -1e-20, 1e18, 3e19, -3e19, float("inf"), float("nan"))
G16_SPECIAL = (0.0, -0.0, 2.0 ** -20, -(2.0 ** -20), 65504.0, -65504.0, float("inf"), float("-inf"), float("nan"))
ZONE = 48  # elements at either end of a tensor that carry the planted classes


def _plant(n):
    """the planted indices of a tensor: both ends (the tail elements are among them), every position of a short tensor"""
    idx = np.arange(n)
    return idx[(idx < ZONE) | (idx >= n - ZONE)]


def tensor_values(n, seed, ghalf):
    """`_tensor_values`, kept for the small tensors that many cases share"""
    return (_tensor_values_cached if n <= 1 << 16 else _tensor_values)(n, seed, ghalf)


def _tensor_values(n, seed, ghalf):
    """-> (p, g, m, v) of one tensor, read-only arrays.  Ordinary values: g = +-10^[-4, 4) (eight decades; fp16: 10^[-4, 4)
    rounded to half), a third of them exactly 0 together with m = v = 0 in runs of four elements (dead groups), m = +-1e-2-ish,
    v = m^2-ish, p in [-1, 1).  Planted at both ends, cycling with the seed: the special gradients, m and v in {0, denormal,
    ordinary} and p in {+0, -0, ordinary, 1e30}; every fourth planted element keeps an ordinary gradient."""
    r = np.random.default_rng(1000003 * seed + n)
    p = r.uniform(-1, 1, n).astype(f32)
    g = (r.choice([-1.0, 1.0], n) * 10.0 ** r.uniform(-4, 4, n)).astype(f32)
    m = (r.standard_normal(n) * 1e-2).astype(f32)
    v = (r.standard_normal(n) ** 2 * 1e-4).astype(f32)
    run = np.repeat(r.random((n + 3) // 4) < 1 / 3, 4)[:n]  # dead groups (rows never addressed)
    g[run], m[run], v[run] = 0, 0, 0
    special = G16_SPECIAL if ghalf else G32_SPECIAL
    for j in _plant(n).tolist():
        c = (j + seed) % (len(special) + 4)
        if c < len(special):
            g[j] = special[c]
        else:
            g[j] = f32(r.choice([-1.0, 1.0]) * 10.0 ** r.uniform(-4, 4))
        mc, vc, pc = (j * 7 + seed) % 3, (j * 5 + seed // 3) % 3, (j * 11 + seed) % 4
        m[j] = (0.0, DENORMAL32 * (-1) ** j, r.standard_normal() * 1e-2)[mc]
        v[j] = (0.0, DENORMAL32, r.standard_normal() ** 2 * 1e-4 + 1e-12)[vc]
        if pc != 2:
            p[j] = (0.0, -0.0, 0.0, 1e30)[pc]
    with np.errstate(all="ignore"):
        g = g.astype(f16) if ghalf else g
    for x in (p, g, m, v):
        x.setflags(write=False)
    return p, g, m, v


_tensor_values_cached = functools.lru_cache(maxsize=256)(_tensor_values)


# ---- cases ---------------------------------------------------------------------------------------------------------------
SENTINEL = 64  # elements between two tensors of a slab, and at both ends
Patch = namedtuple("Patch", "tensor field start values")  # field in p g m v image; written after generation
Case = namedtuple("Case", "name ns steps ghalf image hyper seed patches",
                  defaults=((),))

H_PLAIN = Hyper(grad_scale=0.5)
H_DECAY = Hyper(wd=1e-2, grad_scale=0.5)
H_DEV = Hyper(wd=1e-2, grad_scale=0.5 / 1024.0)  # host_grad_scale 0.5 over a device scale of 1024, a device lr


def case(name, ns, steps=None, ghalf=False, image=False, hyper=H_PLAIN, seed=0, patches=()):
    ns = tuple(int(n) for n in ns)
    many = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x,) * len(ns)  # noqa: E731
    steps = tuple(range(1, len(ns) + 1)) if steps is None else many(steps)
    return Case(name, ns, steps, many(ghalf), many(image), hyper, seed, tuple(patches))


class Slabs:
    """Every tensor of a case as a 16-byte aligned slice of one buffer per kind (p, m, v, g32 fp32; g16, image fp16), with
    SENTINEL or more sentinel elements before, between and after.  Every tensor owns its range in EVERY buffer, used or
    not (an fp32-gradient tensor's range of g16, an image-less tensor's range of image): a call must not write those."""
    KINDS = ("p", "m", "v", "g32", "g16", "image")

    def __init__(self, c):
        self.case = c
        off, self.off = SENTINEL, []
        for n in c.ns:
            self.off.append(off)
            off += (n + SENTINEL + 7) // 8 * 8  # multiples of 8 elements: 16 bytes for the fp16 buffers too
        self.size = off + SENTINEL
        pos = np.arange(self.size)
        fill32 = (f32(-7.0) - (pos % 251).astype(f32) * f32(0.125))
        self.a = {k: fill32.copy() for k in ("p", "m", "v", "g32")}
        self.a["g16"], self.a["image"] = fill32.astype(f16), (fill32 * f32(0.5)).astype(f16)
        for k, n in enumerate(c.ns):
            p, g, m, v = tensor_values(n, c.seed + 17 * k, bool(c.ghalf[k]))
            s = slice(self.off[k], self.off[k] + n)
            self.a["p"][s], self.a["m"][s], self.a["v"][s] = p, m, v
            self.a["g16" if c.ghalf[k] else "g32"][s] = g
            if c.image[k]:  # a stale image: the call has to write every element it updates
                self.a["image"][s] = half_rn(p * f32(1.5) + f32(0.25))
        for pt in c.patches:
            kind = ("g16" if c.ghalf[pt.tensor] else "g32") if pt.field == "g" else pt.field
            o = self.off[pt.tensor] + pt.start
            assert pt.start + len(pt.values) <= c.ns[pt.tensor]
            self.a[kind][o:o + len(pt.values)] = np.asarray(pt.values, self.a[kind].dtype)

    def view(self, kind, k):
        return self.a[kind][self.off[k]:self.off[k] + self.case.ns[k]]

    def g(self, k):
        return self.view("g16" if self.case.ghalf[k] else "g32", k)


VARIANTS = ("neighbour_args", "tail_short", "no_second_pass", "dead_no_decay", "image_trunc", "scale_after_m", "step_minus_1",
            "half_swap") + tuple(f"skip_ignores_{f}{lane}" for f in "gmv" for lane in range(4))


def case_args(c, k, variant=None):
    h = c.hyper
    if variant == "neighbour_args":
        live = [j for j, n in enumerate(c.ns) if n > 0]
        k = live[(live.index(k) + 1) % len(live)]
    step = c.steps[k] - 1 if variant == "step_minus_1" else c.steps[k]
    return adam_args(step, h.lr, h.b1, h.b2, h.eps, h.wd, h.grad_scale)


def expected(c, slabs=None, variant=None, single=False):
    """the slabs after one call: {kind: array}.  variant: the slabs a kernel with that mistake would leave."""
    slabs = slabs or Slabs(c)
    out = {k: a.copy() for k, a in slabs.a.items()}
    plans, _ = launch_plan(c.ns, single=single)
    for k, n in enumerate(c.ns):
        if n == 0:
            continue
        a = case_args(c, k, variant)
        p, g, m, v = slabs.view("p", k), slabs.g(k), slabs.view("m", k), slabs.view("v", k)
        img = slabs.view("image", k) if c.image[k] else None
        ev = variant if variant in ("dead_no_decay", "image_trunc", "scale_after_m", "half_swap") else None
        p1, m1, v1, i1 = replay(p, g, m, v, a, img, variant=ev)
        keep = np.zeros(n, bool)  # elements the wrong kernel leaves alone
        n4 = n // 4 * 4
        if variant == "tail_short":  # the tail lanes address the last full group instead: it is updated twice, the tail never
            keep[n4:] = True
            if n4 >= 4 and n > n4:
                s = slice(n4 - 4, n4 - 4 + (n - n4))
                q = replay(p1[s], g[s], m1[s], v1[s], a, None if i1 is None else i1[s])
                p1[s], m1[s], v1[s] = q[0], q[1], q[2]
                if i1 is not None:
                    i1[s] = q[3]
        if variant == "no_second_pass":
            keep[min(plans[k].blocks * 256 * 4, n4):n4] = True
        if variant and variant.startswith("skip_ignores_") and a.decay == f32(1) and a.eps > 0:
            field, lane = variant[-2], int(variant[-1])
            z = np.stack([np.asarray(x[:n4]).astype(f32).reshape(-1, 4) == 0 for x in (g, m, v)])  # [3, groups, 4]
            z[{"g": 0, "m": 1, "v": 2}[field], :, lane] = True
            keep[:n4] |= np.repeat(z.all((0, 2)), 4)
        p1, m1, v1 = np.where(keep, p, p1), np.where(keep, m, m1), np.where(keep, v, v1)
        o = slice(slabs.off[k], slabs.off[k] + n)
        out["p"][o], out["m"][o], out["v"][o] = p1, m1, v1
        if i1 is not None:
            out["image"][o] = np.where(keep, img, i1)
    return out


def differs(c, variant, single=False):
    """does the wrong kernel `variant` leave other slabs than the right one on this case?"""
    s = Slabs(c)
    good, bad = expected(c, s, single=single), expected(c, s, variant, single=single)
    return any(mismatches(bad[k], good[k]).size for k in Slabs.KINDS)


# ---- the case lists ------------------------------------------------------------------------------------------------------
SMALL_NS = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1028)
ALONE_NS = (4194304, 4194308, 4194304 + 4 * 300 + 3)  # passes of the first / last lane at the 4096 cap: 1/1, 2/1, 2/1 + tail
COMPANY_NS = (1048576, 1048580, 1048576 + 4 * 300 + 3)  # the same at the 1024 cap of a shared launch
COMPANION = 37  # the second live tensor of a shared launch


def small_cases(route):
    """one tensor per call: every small length x gradient dtype x image, where the route allows them; steps 1 .. 10"""
    out = []
    for i, n in enumerate(SMALL_NS):
        for ghalf in ((False,) if route == "step" else (False, True)):
            for image in ((False,) if route == "step" else (False, True)):
                out.append(case(f"n{n}-{'h' if ghalf else 'f'}{'-img' if image else ''}", [n], steps=[i + 1], ghalf=ghalf,
                                image=image, hyper=H_DECAY if i % 2 else H_PLAIN, seed=3 + i))
    return out


def big_cases(route):
    """one case per big length and gradient dtype; the fp16 ones carry an image"""
    out = []
    for i, n in enumerate(ALONE_NS):
        for ghalf in ((False,) if route == "step" else (False, True)):
            out.append(case(f"alone{n}-{'h' if ghalf else 'f'}", [n], steps=[3 + i], ghalf=ghalf, image=ghalf, seed=40 + i))
    if route != "step":
        for i, n in enumerate(COMPANY_NS):
            for ghalf in (False, True):
                out.append(case(f"company{n}-{'h' if ghalf else 'f'}", [COMPANION, n], steps=[7, 2 + i],
                                ghalf=[not ghalf, ghalf], image=[False, ghalf], seed=50 + i))
    return out


_MIX = (260, 1, 4100, 1027, 2, 1024, 9, 2051, 3, 516, 1030, 4, 7, 3077, 1025, 5, 12, 1029, 2048, 6, 1026, 258, 1031, 11, 8)


def _mixed(live):
    """`live` tensors of mixed lengths: one and several workgroups, tails 0 .. 3"""
    return [_MIX[j % len(_MIX)] + 4 * (j // len(_MIX)) for j in range(live)]


def batch_cases():
    """23, 24, 25, 48, 49 live tensors, each with its own step count, alternating gradient dtypes and image presence;
    empties first, in the middle, at list index 24 and last; only empties; 24 live ones followed by empties"""
    out = []
    for live in (23, 24, 25, 48, 49):
        ns = _mixed(live)
        out.append(case(f"live{live}", ns, ghalf=[j % 2 == 1 for j in range(live)], image=[j % 3 == 0 for j in range(live)],
                        hyper=H_DECAY if live % 2 else H_PLAIN, seed=60 + live))
    ns = _mixed(30)
    for at in (0, 12, 24, len(ns) + 3):  # first, middle, list index 24, last (after the three insertions before it)
        ns.insert(at, 0)
    assert ns[0] == 0 and ns[24] == 0 and ns[-1] == 0
    out.append(case("empties-between", ns, ghalf=[j % 2 == 0 for j in range(len(ns))], image=[j % 3 == 0 for j in range(len(ns))],
                    seed=91))
    out.append(case("only-empties", [0, 0, 0], seed=92))
    out.append(case("24-then-empties", _mixed(24) + [0, 0, 0], ghalf=[j % 2 == 1 for j in range(27)],
                    image=[j % 3 == 1 for j in range(27)], seed=93))
    return out


DEAD_N, DEAD_GROUP = 1031, 130  # 257 groups of four: two workgroups, group 130 in the first; a tail of three


def _dead_patches(nonzero=None, tail=True):
    """group DEAD_GROUP (and the tail) with g = m = v = 0, p = (-0, 0.3, -1.7, +0) and the image at half(p);
    nonzero = (field, lane): that one value of the group is not zero"""
    s = 4 * DEAD_GROUP
    pv = (-0.0, 0.3, -1.7, 0.0)
    vals = {"g": [0.0] * 4, "m": [0.0] * 4, "v": [0.0] * 4}
    if nonzero:
        vals[nonzero[0]][nonzero[1]] = {"g": -1e-3, "m": -1e-3, "v": 1e-6}[nonzero[0]]
    pt = [Patch(0, "p", s, pv), Patch(0, "image", s, tuple(half_rn(pv).tolist()))] + [Patch(0, f, s, tuple(x)) for f, x in vals.items()]
    if tail:
        t = DEAD_N // 4 * 4
        pt += [Patch(0, f, t, (0.0, 0.0, 0.0)) for f in "gmv"]
        pt += [Patch(0, "p", t, pv[:3]), Patch(0, "image", t, tuple(half_rn(pv[:3]).tolist()))]
    return pt


def dead_cases(ghalf=False):
    """-> {name: case}: all-zero; the twelve one-non-zero patterns; all-zero under AdamW; all-zero with eps = 0 and 1e-50"""
    mk = lambda name, hyper, nz=None: case(name, [DEAD_N], steps=[4], ghalf=ghalf, image=True, hyper=hyper, seed=70,  # noqa: E731
                                           patches=_dead_patches(nz))
    out = {"zero": mk("dead-zero", H_PLAIN), "decay": mk("dead-decay", H_DECAY),
           "eps0": mk("dead-eps0", H_PLAIN._replace(eps=0.0)), "eps1e-50": mk("dead-eps1e-50", H_PLAIN._replace(eps=1e-50))}
    for f in "gmv":
        for lane in range(4):
            out[f"one-{f}{lane}"] = mk(f"dead-one-{f}{lane}", H_PLAIN, (f, lane))
    return out


def error_case():
    """30 tensors for the nothing-touched tests (the 28th is the one the test spoils)"""
    return case("errors30", _mixed(30), ghalf=[j % 2 == 1 for j in range(30)], image=[j % 3 == 0 for j in range(30)], seed=95)


def all_cases():
    """every Adam case of the GPU tests with the route(s) that run it: [(case, single)]"""
    out = [(c, True) for c in small_cases("step") + big_cases("step")]
    out += [(c, False) for c in small_cases("many") + big_cases("many") + batch_cases() + list(dead_cases().values())
            + list(dead_cases(True).values()) + [error_case(), dev_lr_decay_case(), dev_scales_case()]]
    return out


def dev_lr_decay_case():
    """a device learning rate (an fp32 value, so not 1e-2 itself) together with weight decay"""
    return case("dev-lr-decay", [1029, 6, 2051], ghalf=[False, True, False], image=[False, True, False],
                hyper=Hyper(lr=float(f32(7e-3)), wd=1e-2), seed=80)


def dev_scales_case():
    """host_grad_scale = 0.5 together with a device scale of 1024"""
    return case("dev-scales", [1027, 5, 2050], ghalf=[True, False, True], image=[True, False, False], hyper=H_DEV, seed=81)


# ---- nonfinite_check -----------------------------------------------------------------------------------------------------
CHECK_NS = {"fp32-company": 4 * (5 * 262144 + 700) + 3, "fp16-company": 8 * (5 * 262144 + 700) + 7,
            "fp32-alone": 4 * (5 * 1048576 + 700) + 3}


def check_positions(name):
    """-> (n, half, element indices to poison one at a time, plan).  Each of the four unrolled loads and the first remainder
    iteration for lane 0, a middle lane and the last lane, the second remainder iteration for lanes 0, 350 and 699, each in
    every dword (halfword) of the 16 bytes; every tail element."""
    n, half = CHECK_NS[name], name.startswith("fp16")
    company = name.endswith("company")
    ns = [n, COMPANION] if company else [n]
    plan = launch_plan(ns, check_half=[half] * len(ns))[0][0]
    per, stride = (8 if half else 4), plan.blocks * 256
    where = []
    for it in range(5):
        for lane in (0, stride // 2 + 37, stride - 1):
            where += [(lane + it * stride) * per + e for e in range(per)]
    for lane in (0, 350, 699):
        where += [(lane + 5 * stride) * per + e for e in range(per)]
    where += list(range(n - plan.tail, n))
    assert max(where) == n - 1 and len(set(where)) == len(where)
    return n, half, where, plan
