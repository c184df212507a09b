"""Integer operand families, float64 references and per-element checkers of the RGB decoder's kernels (csrc/decoder.hip):
tests/test_decoder_refs_host.py on the CPU, tests/test_gpu_decoder_exact.py on the GPU.

EXACT CASES.  Every layer but BatchNorm's normalisation and the sigmoid is a sum of products of fp16 operands accumulated
in fp32.  With operands in {-1, 0, 1} (features of the first layer: small integers) every product and every partial sum of
ANY summation order is an integer no larger than S = sum |a||b| + |bias|.  Integers up to 2^24 are fp32 numbers, integers
up to 2048 = 2^11 are fp16 numbers, so with S <= 2048 where the result is stored as fp16 and S < 2^24 where it stays fp32
the kernel has no rounding to do: its output equals the float64 reference BIT FOR BIT.  The builders check S on the
reference run on absolute values (`exact_fp16`, `exact_fp32`) and raise when a family breaks it; nothing is skipped.  With
a working scale 1/S' = 2^-k (ops_decoder.grad_scale) a parameter gradient is prefill + 2^-k * integer: still exact while
2^k * |result| < 2^24 (`exact_fp32(..., lsb=2^-k)`).

BOUNDED CASES (`assert_within`).  u32 = 2^-24 is fp32's unit roundoff, gamma(K, u) = K u / (1 - K u) bounds any fp32
evaluation of a K-term sum relative to the sum of absolute values (Higham, Accuracy and Stability, Lemma 3.1).  No bound
below is measured; the observed err / bound is recorded in tests/test_gpu_decoder_exact.py for the reader.
  * a sum of K products rounded once to fp16: 2^-11 |ref| + 2^-25 + gamma(K, u) sum |a||b| (half an fp16 ulp of a normal
    result, half the spacing 2^-24 of the subnormals, the accumulation).  Where the sum runs on the matrix cores u = 2^-23
    is taken, not 2^-24: their internal adder is not documented to round to nearest.  This is an ASSUMPTION, not a fact.
  * rgb_fwd, a = bias + 32 fmaf's, rgb = 1 / (1 + __expf(-a)): |da| <= gamma(33, u32) (sum |h||w| + |bias|).  __expf is
    v_exp_f32 (1 ulp) on the fp32 product -a log2(e): the published bound for this intrinsic is 2 + floor(|1.4427 a|) ulp,
    i.e. relative eps_e = (2 + |1.4427 a|) 2^-23.  d sigmoid / da = s (1 - s) and d sigmoid / d ln e = -s (1 - s), so both
    enter as s (1 - s) (|da| + eps_e); the add 1 + e (u32) and the division (2.5 ulp for a division that is not correctly
    rounded, 2.5 * 2^-23) are relative errors of s itself:  s (1 - s) (|da| + eps_e) + s (u32 + 2.5 * 2^-23) + 2^-126.
  * rgb_bwd, dl = ((drgb up) r) (1 - r): four roundings, relative gamma(4, u32).  grad_h = fp16 of two fmaf's and a product
    of it: the fp16 formula with K = 8, u32.  grad_weight / grad_bias: n terms summed in fp32 in a fixed tree, then scaled
    and added to the buffer: gamma(n + 8, u32) sum |dl||h| + u32 |result| (valid for ANY order of the n terms).
  * bn_finalize: statistics in double, each coefficient rounded once, scale and shift by one more fp32 operation: 2 fp32 ulps
    (`ulps32`).
  * bn_bwd: sum g and sum g c are fp32 sums of at most K = ceil(n8 / (256 blocks)) + 64 terms per chain (the thread's
    grid-stride chain, then 64 partials in LDS; the blocks are added in double), blocks = min(1024, ceil(n8 / 4096)):
    e1 = gamma(K) sum |g|, e2 = gamma(K + 1) sum |g c|.  d dgamma = rstd (e2 + |mean| e1); A is exact to u32, dB = A rstd
    d dgamma / count, dC = A e1 / count + dB |mean|, all three then rounded to fp32; grad_c is the fp16 of two fmaf's:
    2^-11 |ref| + 2^-25 + 4 u32 (|A g| + |B c| + |C|) + |c| dB + dC.
  * bn_act / add_masked: no bound, the fp64 REPLAY of the rounding chain (fma -> fp16 -> fp16 add of the skip -> fp16 ->
    ReLU) bit for bit.  The fma is rounded ONCE, from the exact value to fp16 (`round_to_fp16`): the kernel's
    fmaf + conversion compiles to the mixed-precision v_fma_mixlo_f16, which does not round to fp32 in between (a chain
    that did would differ on 1 element in 2^13, those whose fp32 rounding lands on an fp16 tie).  Exempt are elements whose
    pre-rounding value lies within 2^-30 (relative) of the midpoint of two fp16 numbers: the float64 product-sum of the
    replay is itself rounded there.  `rounding_exempt` counts those from the reference alone and raises at 1 in 10^4.  Only the fma needs this: the sum of two fp16 numbers (the skip, add_masked) is
    the same two IEEE operations in the replay as in the kernel (fp32 add, round to fp16), ties included, so nothing is
    exempt there."""
import functools
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U_MFMA = 2.0 ** -23  # assumed: the matrix core's adder may truncate (see above)


# (B, H, W) of the 7x7 convolution for rows-per-wave R; 1 pixel, < 1 tile, > 1 tile in both directions, 3 and 4 column tiles
def conv_shapes(R):
    return [(1, 1, 1), (1, 4 * R - 1, 31), (2, 4 * R + 1, 33), (1, 8 * R, 65), (2, 7, 97)]


WGRAD_SHAPES = [(3, 32, 32), (1, 5, 17), (2, 20, 50), (45, 100, 17), (1, 16, 97), (2, 9, 130),
                (1, 8, 15), (1, 8, 16), (1, 8, 31), (1, 8, 33)]
UP_SHAPES = [(1, 1, 1), (1, 1, 5), (2, 10, 12), (1, 3, 33)]
UP_SHAPE_CAPPED = (1, 257, 511)  # 131,327 pixels: past 1024 workgroups x 4 waves x 32 pixels
IN_CINS = [1, 5, 47, 48, 64]
IN_NS = [1, 63, 64, 65, 130]
RGB_NS = [1, 255, 256, 257, 1023, 1024, 1025, 4099]
BN_PARTIAL_NS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 1000]
EW_PIXELS = [1, 63, 64, 65, 8193]
BN_BWD_PIXELS_CAPPED = 1024 * 1024 + 3


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


# ---- integer operand builders ------------------------------------------------------------------------------------------
def ints(shape, lo, hi, seed):
    """seeded integers in [lo, hi] as float64"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def act_pm1(shape, seed):
    """activations / gradients in {-1, 0, 1}: NHWC fp16 [..., 32]"""
    return ints(tuple(shape) + (32,), -1, 1, seed).half()


def weight_pm1(shape, seed):
    return ints(shape, -1, 1, seed).float()


def bias_int(n, seed, lo=-8, hi=8):
    return ints((n,), lo, hi, seed).float()


def exact_fp16(abs_sum, what):
    """raise unless every magnitude that can occur while the sums behind `abs_sum` are formed is an fp16 number"""
    m = float(abs_sum.max()) if abs_sum.numel() else 0.0
    if m > 2048:
        raise ValueError(f"{what}: sum |a||b| reaches {m} > 2048, not exact in fp16")
    return m


def exact_fp32(abs_sum, what, lsb=1.0):
    m = float(abs_sum.max()) if abs_sum.numel() else 0.0
    if m / lsb >= 2.0 ** 24:
        raise ValueError(f"{what}: sum |a||b| reaches {m} (lsb {lsb}), not exact in fp32")
    return m


# ---- float64 references ------------------------------------------------------------------------------------------------
def nchw(x):
    return x.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous()


def d64(t):
    return t.detach().cpu().double()


def h16(t):
    """the value an fp32 parameter carries once the kernel has rounded it to fp16"""
    return t.detach().cpu().float().half().double()


def conv7_fwd(x, w, bias=None):
    """x NHWC, w [32, 32, 7, 7] (torch Conv2d) -> NHWC float64"""
    return nhwc(F.conv2d(nchw(x), d64(w), None if bias is None else d64(bias), padding=3))


def conv7_grads(x, w, g):
    """-> (input gradient NHWC, weight gradient [32, 32, 7, 7], bias gradient [32]) of conv2d(x, w, padding 3) under g"""
    xr, wr = nchw(x).requires_grad_(), d64(w).requires_grad_()
    br = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, padding=3).backward(nchw(g))
    return nhwc(xr.grad), wr.grad, br.grad


def up_fwd(x, w, bias):
    """ConvTranspose2d(kernel = stride = 3): x NHWC [B, H, W, 32], w [32, 32, 3, 3] (in, out, ky, kx) -> [B, 3H, 3W, 32]"""
    return nhwc(F.conv_transpose2d(nchw(x), d64(w), d64(bias), stride=3))


def up_grads(x, w, g):
    xr, wr = nchw(x).requires_grad_(), d64(w).requires_grad_()
    br = torch.zeros(w.shape[1], dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(xr, wr, br, stride=3).backward(nchw(g))
    return nhwc(xr.grad), wr.grad, br.grad


def in_fwd(feat, w, bias):
    """Conv2d(cin, 32, 1) + ReLU on feature rows [n, cin]; w [32, cin]; operands as the kernel rounds them"""
    return torch.relu(h16(feat) @ h16(w).reshape(32, -1).t() + d64(bias))


def in_bwd(feat, w, h_stored, dh):
    """the mask is the STORED activation's -> (dfeat [n, cin], grad_weight [32, cin], grad_bias [32])"""
    g = d64(dh) * (d64(h_stored) > 0)
    return g @ h16(w).reshape(32, -1), g.t() @ h16(feat), g.sum(0)


def rgb_fwd(h, w, bias):
    """Conv2d(32, 3, 1) + Sigmoid on h [..., 32] -> (rgb [n, 3], pre-activation a, sum |h||w| + |bias|)"""
    hh, ww = d64(h).reshape(-1, 32), h16(w).reshape(3, 32)
    a = hh @ ww.t() + d64(bias)
    return torch.sigmoid(a), a, hh.abs() @ ww.abs().t() + d64(bias).abs()


def rgb_fwd_bound(s, a, abs_sum):
    eps_e = (2.0 + 1.4427 * a.abs()) * 2.0 ** -23
    return s * (1 - s) * (gamma(33) * abs_sum + eps_e) + s * (U32 + 2.5 * 2.0 ** -23) + 2.0 ** -126


def rgb_bwd(h, rgb, drgb, w):
    """-> (grad_h [n, 32], grad_weight [3, 32], grad_bias [3]) and the same three on absolute values"""
    hh, ww, r = d64(h).reshape(-1, 32), h16(w).reshape(3, 32), d64(rgb).reshape(-1, 3)
    dl = d64(drgb).reshape(-1, 3) * r * (1 - r)
    return (dl @ ww, dl.t() @ hh, dl.sum(0)), (dl.abs() @ ww.abs(), dl.abs().t() @ hh.abs(), dl.abs().sum(0))


def bn_stats(c):
    """channel statistics of c [..., 32]: mean, biased variance, unbiased variance (torch's running_var)"""
    v = d64(c).reshape(-1, 32)
    n = v.shape[0]
    mean = v.mean(0)
    var = (v - mean).square().mean(0)
    return mean, var, var * (n / (n - 1) if n > 1 else 1.0)


def bn_finalize(part, count, gamma_, beta, eps, momentum, running_mean, running_var):
    """per-workgroup partials [n, 64] (sums, sums of squares) -> (coef [4, 32] = scale, shift, mean, rstd; new running
    mean; new running variance), all float64, with the kernel's one documented fp32 step: shift uses the fp32 mean"""
    tot = d64(part).sum(0)
    mean = tot[:32] / count
    var = (tot[32:] / count - mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    sc = d64(gamma_) * rstd
    shift = d64(beta) - mean.float().double() * sc
    m = float(torch.tensor(momentum, dtype=torch.float32))
    unb = var * count / (count - 1 if count > 1 else 1)
    return torch.stack([sc, shift, mean, rstd]), (1 - m) * d64(running_mean) + m * mean, (1 - m) * d64(running_var) + m * unb


def bn_bwd(dout, act, c, gamma_, coef):
    """the affine BatchNorm backward dc = A g + B c + C with g = dout (act > 0), mean and rstd as coef holds them ->
    dict(dc, dgamma, dbeta, bound_dc, bound_dgamma, bound_dbeta) for the kernel's launch plan (see the module docstring)"""
    g = (d64(dout) * (d64(act) > 0)).reshape(-1, 32)
    v = d64(c).reshape(-1, 32)
    n = v.shape[0]
    mean, rstd = d64(coef)[2], d64(coef)[3]
    sum_g, sum_gc = g.sum(0), (g * v).sum(0)
    dg = rstd * (sum_gc - mean * sum_g)
    A = d64(gamma_) * rstd
    B = -A * rstd * dg / n
    C = -A * sum_g / n - B * mean
    dc = A * g + B * v + C
    n8 = 4 * n
    blocks = min(1024, max(1, -(-n8 // 4096)))
    K = -(-n8 // (256 * blocks)) + 64
    e1, e2 = gamma(K) * g.abs().sum(0), gamma(K + 1) * (g * v).abs().sum(0)
    ddg = rstd * (e2 + mean.abs() * e1)
    dB = A.abs() * rstd * ddg / n + U32 * B.abs()
    dC = A.abs() * e1 / n + dB * mean.abs() + U32 * C.abs()
    mag = (A * g).abs() + (B * v).abs() + C.abs()
    bound_dc = 2.0 ** -11 * dc.abs() + 2.0 ** -25 + 4 * U32 * mag + U32 * (A * g).abs() + v.abs() * dB + dC
    return dict(dc=dc.reshape(c.shape), dgamma=dg, dbeta=sum_g, bound_dc=bound_dc.reshape(c.shape),
                bound_dgamma=ddg + 2 * U32 * dg.abs(), bound_dbeta=e1 + 2 * U32 * sum_g.abs())


def _fp16_midpoint_distance(t):
    """relative distance of float64 t from the nearest midpoint of two neighbouring fp16 numbers"""
    a = t.abs()
    e = torch.floor(torch.log2(a.clamp(min=2.0 ** -14))).clamp(min=-14.0)
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)
    q = a / ulp
    return ((q - torch.floor(q)) - 0.5).abs() * ulp / a.clamp(min=2.0 ** -24)


def round_to_fp16(t):
    """float64 -> the nearest fp16 number (ties to even) in ONE rounding; torch's own conversion goes through fp32"""
    e = torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -14))).clamp(min=-14.0)
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)
    return (torch.round(t / ulp) * ulp).half()


def rounding_exempt(pre, what):
    """elements whose exact pre-rounding value lies within 2^-30 (relative) of an fp16 rounding boundary; raises when they
    are 1 in 10^4 of the input or more (decided from the reference alone)"""
    ex = _fp16_midpoint_distance(pre) <= 2.0 ** -30
    if ex.sum().item() * 10 ** 4 >= max(pre.numel(), 10 ** 4):
        raise ValueError(f"{what}: {int(ex.sum())} of {pre.numel()} elements sit on an fp16 rounding boundary")
    return ex


def bn_act(c, coef, skip=None):
    """relu(bn(c) [+ skip]) with the kernel's rounding chain replayed -> (fp16 result, exempt mask)"""
    cf = d64(coef)
    q = torch.arange(32)
    pre = d64(c) * cf[0][q] + cf[1][q]
    y = round_to_fp16(pre)
    ex = rounding_exempt(pre, "bn_act")
    if skip is not None:
        s = skip.detach().cpu()
        y = (y.float() + s.float()).half()
    return torch.relu(y.float()).half(), ex


def add_masked(a, dout, act):
    """mode 1 of bn_bwd_apply: fp16(a + dout (act > 0)), the add in fp32 -> (fp16 result, None: nothing is exempt)"""
    a, dout, act = a.detach().cpu(), dout.detach().cpu(), act.detach().cpu()
    g = torch.where(act.float() > 0, dout.float(), torch.zeros((), dtype=torch.float32))
    return (a.float() + g).half(), None


def fp16_sum_bound(ref, abs_sum, k, u):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25 + gamma(k, u) * abs_sum


# ---- launch plans restated (what the C ABI does not answer) --------------------------------------------------------------
def wgrad_tasks(w):
    """(X blocks, G blocks) of 32 pixels that conv7_wgrad_kernel stages per image row: its 7 waves prefetch one task each,
    the unprefetched loop runs when the sum exceeds 7"""
    nkb = (w + 15) // 16
    return (16 * nkb + 8 + 31) // 32, (16 * nkb + 31) // 32


def wgrad_lds_bytes(w):
    def pitch(halves):
        n = (halves + 7) // 8
        return 8 * (n + 1 - n % 2)
    nxb, ngb = wgrad_tasks(w)
    return 2 * (8 * 32 * pitch(32 * nxb) + 2 * 32 * pitch(32 * ngb))


def conv_tile_sums(out, R):
    """per-workgroup (sum |v|, sum v^2) of a convolution output NHWC [B, H, W, 32] cut into 4R x 32 tiles: the largest
    magnitude a statistics partial can pass through"""
    v = d64(out)
    B, H, W, _ = v.shape
    th = 4 * R
    s1 = s2 = 0.0
    for y0 in range(0, H, th):
        for x0 in range(0, W, 32):
            t = v[:, y0:y0 + th, x0:x0 + 32]
            s1 = max(s1, float(t.abs().sum((1, 2)).max()))
            s2 = max(s2, float(t.square().sum((1, 2)).max()))
    return s1, s2


# ---- checkers ------------------------------------------------------------------------------------------------------------
def assert_equal(got, want, what, exempt=None):
    """bit-for-bit (as values: -0 == +0) with the first offender reported"""
    g, w = got.detach().cpu(), want.detach().cpu().to(got.dtype)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    bad = g != w
    if exempt is not None:
        bad &= ~exempt
    if bad.any():
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ; first at {i}: got {g[i].item()!r}, "
                             f"want {w[i].item()!r}")


def assert_within(got, ref64, bound, what):
    """|got - ref64| <= bound element by element -> the largest err / bound (for the record)"""
    g, r = d64(got).reshape(ref64.shape), ref64
    b = torch.as_tensor(bound, dtype=torch.float64).expand(r.shape)
    err = (g - r).abs()
    bad = ~(err <= b)  # a nan fails
    if bad.any():
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements out of bound; first at {i}: got {g[i].item()!r}, "
                             f"want {r[i].item()!r}, bound {b[i].item():.3e}")
    return float((err / b.clamp(min=1e-300)).max()) if g.numel() else 0.0


def ulps32(got, ref64):
    """|got - ref64| in fp32 ulps of ref64, element by element"""
    r = ref64.abs().clamp(min=2.0 ** -126)
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(r)) - 23)
    return (d64(got).reshape(ref64.shape) - ref64).abs() / ulp


def expected_grad_scale(amax):
    """(S, 1/S) of ops_decoder.grad_scale for a finite maximum amax: S = 2^-e with amax = f 2^e, f in [0.5, 1), e clamped"""
    e = 0
    if amax > 0:
        e = max(-60, min(60, -math.frexp(amax)[1]))
    return 2.0 ** e, 2.0 ** -e


# ---- exact cases: operands, references, representability -----------------------------------------------------------------
def wgrad_plan(b, h):
    """(rows per strip, strips per image) of conv7_wgrad_kernel: equal strips of at least 16 rows, more once b * h > 4096"""
    rps = min(max(16, -(-b * h // 256)), h)
    return rps, -(-h // rps)


@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, seed=31):
    """the 7x7 convolution on integers: x, w, bias, g and the exact forward output and input gradient (fp16-exact)"""
    x, g = act_pm1((B, H, W), seed), act_pm1((B, H, W), seed + 1)
    w, bias = weight_pm1((32, 32, 7, 7), seed + 2), bias_int(32, seed + 3)
    what = f"conv7x7 {(B, H, W)}"
    exact_fp16(conv7_fwd(x.abs(), w.abs(), bias.abs()), what + " forward")
    exact_fp16(conv7_grads(g.abs(), w.abs(), g.abs())[0], what + " input gradient")
    return dict(x=x, g=g, w=w, bias=bias, out=conv7_fwd(x, w, bias), dx=conv7_grads(x, w, g)[0])


@functools.lru_cache(maxsize=None)
def wgrad_case(B, H, W, seed=41, prefill=3.0, lsb=1.0):
    """the 7x7 convolution's weight / bias gradient on integers, accumulated into buffers pre-filled with an integer"""
    x, g = act_pm1((B, H, W), seed), act_pm1((B, H, W), seed + 1)
    w0 = torch.zeros((32, 32, 7, 7))
    _, dw, db = conv7_grads(x, w0, g)
    _, aw, ab = conv7_grads(x.abs(), w0, g.abs())
    exact_fp32(aw + abs(prefill) / lsb, f"conv7x7_wgrad {(B, H, W)} weight", lsb)
    exact_fp32(ab + abs(prefill) / lsb, f"conv7x7_wgrad {(B, H, W)} bias", lsb)
    return dict(x=x, g=g, dw=dw, db=db, prefill=prefill)


@functools.lru_cache(maxsize=None)
def up_case(B, H, W, seed=51):
    """ConvTranspose2d(32, 32, 3, stride 3) on integers: forward, data / weight / bias gradient"""
    x, g = act_pm1((B, H, W), seed), act_pm1((B, 3 * H, 3 * W), seed + 1)
    w, bias = weight_pm1((32, 32, 3, 3), seed + 2), bias_int(32, seed + 3)
    what = f"upsample {(B, H, W)}"
    exact_fp16(up_fwd(x.abs(), w.abs(), bias.abs()), what + " forward")
    adx, adw, adb = up_grads(x.abs(), w.abs(), g.abs())
    exact_fp16(adx, what + " data gradient")
    exact_fp32(adw, what + " weight gradient")
    exact_fp32(adb, what + " bias gradient")
    dx, dw, db = up_grads(x, w, g)
    return dict(x=x, g=g, w=w, bias=bias, out=up_fwd(x, w, bias).half(), dx=dx.half(), dw=dw, db=db)


@functools.lru_cache(maxsize=None)
def in_case(n, cin, seed=61):
    """the first layer on integer features in [-3, 3] (fp32), weights in {-1, 0, 1}"""
    feat, w, bias = ints((n, cin), -3, 3, seed).float(), weight_pm1((32, cin), seed + 1), bias_int(32, seed + 2)
    dh = ints((n, 32), -1, 1, seed + 3).half()
    what = f"conv1x1_in n={n} cin={cin}"
    exact_fp16(in_fwd(feat.abs(), w.abs(), bias.abs()), what + " forward")
    h = in_fwd(feat, w, bias)
    for t, name in zip(in_bwd(feat.abs(), w.abs(), torch.ones_like(h), dh.abs()), ("dfeat", "grad_weight", "grad_bias")):
        exact_fp32(t, f"{what} {name}")
    dfeat, dw, db = in_bwd(feat, w, h, dh)
    return dict(feat=feat, w=w, bias=bias, dh=dh, h=h.half(), dfeat=dfeat, dw=dw, db=db)
