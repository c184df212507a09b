"""Integer operand cases, the int64 reference and the restated launch plans of the MLP kernels (csrc/mlp.hip,
csrc/mlp_chain.hip): tests/test_mlp_refs_host.py on the CPU, tests/test_gpu_mlp_exact.py on the GPU.

WHY BIT EQUALITY.  Both files compute in fp32 throughout: v_mfma_f32_16x16x4_f32 and fp32 adds in registers, in the LDS
merges of the wave partials, in wgrad_merge_kernel and in the fp32 atomics of mlp_wgrad_kernel.  An fp32 operation on two
integers whose exact result is an integer of magnitude < 2^24 returns that integer: nothing is rounded.  Let every operand
be an integer and let S = sum |a||b| (+ |bias|, + |prefill| of an accumulated buffer) be taken over ALL terms of one
output element.  Every partial sum of every subset of the terms, in any order and any grouping, is an integer of
magnitude <= S.  So with S < 2^24 no kernel has a rounding to do, whatever its tile order, its split over waves,
workgroups and sample slices, or the order in which atomics land, and the result is the exact integer: the int64
reference below, bit for bit.  Zero padding of the MFMA tiles adds terms that are 0.  The sums that occur are
  forward            z_l[n][o]  = b_l[o] + sum_i W_l[o][i] a_{l-1}[n][i]        S = |b_l[o]| + sum_i |W_l[o][i]| |a_{l-1}[n][i]|
  data gradient      dH_{l-1}[n][i] = sum_o dZ_l[n][o] W_l[o][i]                S = sum_o |dZ_l[n][o]| |W_l[o][i]|
  weight gradient    dW_l[o][i] += sum_n dZ_l[n][o] a_{l-1}[n][i]               S = |prefill| + sum_n |dZ_l[n][o]| |a_{l-1}[n][i]|
  bias gradient      db_l[o]    += sum_n dZ_l[n][o]                             S = |prefill| + sum_n |dZ_l[n][o]|
  residual head      grad_geo[n][1 + c] = grad_feature[n][c] + grad_x[n][c]     S = |grad_feature[n][c]| + S(grad_x[n][c])
with a_{-1} = x, a_l = relu(z_l), dZ_last = grad_y, dZ_l = dH_l (z_l > 0): the ACTUAL activations and dZ, since those are
the operands the kernels multiply (the data gradient is formed for every unit and masked afterwards, hence dH is bounded
before the mask).  `assert_exact_operands` evaluates every S above for a case and demands max S < 2^24: a condition on
the operands, not a measurement of any kernel.  The ReLU mask is z > 0 on the exact integers; z == 0 occurs (one unit per
hidden layer has a zero weight row and a zero bias, more arise by chance) and must mask.
There is ample room.  The largest S of the largest cases, from the references alone (x, grad_y in [-2, 2]):
  64 -> 64 -> 64 -> 32, n = 70001    8.8e5 (weight gradient)      48 -> 64 -> 64 -> 32, n = 70001    8.2e5
  5 -> 7 -> 3, n = 262149            6.3e5                        3 -> 5 -> 2, n = 131089            2.9e5
against 2^24 = 1.7e7; 32 - 59 % of the hidden units are live, 87 - 98 % of the outputs are nonzero.

The matrix products of the reference are integer products.  Small ones are numpy int64 `@`; large ones run as float64
BLAS products, which are exact on integers below 2^53 (`imatmul` checks that bound on the operands and the integrality of
the result), and tests/test_mlp_refs_host.py compares them with the plain int64 product on sampled rows."""
import functools

import numpy as np
import torch

PREFILL = 3          # every weight / bias gradient buffer starts at this integer: the ABI ACCUMULATES
SENTINEL = -98765.25  # no integer: a reference value never equals it
LIMIT = 2 ** 24


# ---- integer products ----------------------------------------------------------------------------------------------------
def imatmul(a, b):
    """a @ b for int64 matrices, exactly"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape[0] * a.shape[1] * b.shape[1] <= 1 << 24:
        return a @ b
    bound = float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) * a.shape[1]
    assert bound < 2.0 ** 53, "float64 would round this product"
    r = a.astype(np.float64) @ b.astype(np.float64)
    out = r.astype(np.int64)
    assert (out == r).all()
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------
def layer_dims(dims):
    """(in, h, ..., h, out) -> [(out_l, in_l)] per layer; the hidden widths are uniform (nrhip_mlp)"""
    dims = tuple(dims)
    assert len(dims) >= 2 and len(set(dims[1:-1])) <= 1, dims
    return [(dims[l + 1], dims[l]) for l in range(len(dims) - 1)]


def zero_rows(n):
    """rows of grad_y that are exactly zero: a run of two whole 16-row tiles, every 5th row, the last rows"""
    r = np.arange(n)
    z = r % 5 == 4
    if n >= 96:
        z |= (r >= 32) & (r < 64)
    if n >= 8:
        z |= r >= n - min(3, n // 8)
    return z


@functools.lru_cache(maxsize=None)
def case(dims, n, gain=9.6, lo=-2, hi=2, no_bias=(), seed=0):
    """An MLP `dims` = (in, h, ..., out) on n rows of integers.  x and grad_y in [lo, hi]; weights in {-1, 0, 1} with
    density min(1, gain / fan_in) per layer; integer biases in [-2, 2], None for the layers in `no_bias`.  One unit of
    every hidden layer has a zero weight row and no bias: its pre-activation is exactly 0 on every row.
    -> dict: float32 tensors x, grad_y, weights, biases; int64 arrays y, hidden [n, (nl-1) h], z (pre-activations),
    acts (layer inputs), dz, grad_x, dW, db."""
    dims = tuple(dims)
    shapes = layer_dims(dims)
    nl = len(shapes)
    rng = np.random.RandomState((hash_dims(dims) + 7919 * n + 104729 * seed) % (2 ** 31))
    x = rng.randint(lo, hi + 1, size=(n, dims[0])).astype(np.int64)
    gy = rng.randint(lo, hi + 1, size=(n, dims[-1])).astype(np.int64)
    gy[zero_rows(n)] = 0
    W, B = [], []
    for l, (o, i) in enumerate(shapes):
        w = rng.randint(0, 2, size=(o, i)) * 2 - 1
        w = (w * (rng.random_sample((o, i)) < min(1.0, gain / i))).astype(np.int64)
        b = None if l in no_bias else rng.randint(-2, 3, size=(o,)).astype(np.int64)
        if l < nl - 1:  # the unit whose pre-activation is exactly 0 everywhere (it still feeds the next layer's columns)
            k0 = (3 + 5 * l) % o
            w[k0] = 0
            if b is not None:
                b[k0] = 0
        W.append(w), B.append(b)
    acts, z = [x], []
    for l in range(nl):
        t = imatmul(acts[-1], W[l].T)
        if B[l] is not None:
            t = t + B[l]
        z.append(t)
        if l < nl - 1:
            acts.append(np.maximum(t, 0))
    dz, dW, db = [None] * nl, [None] * nl, [None] * nl
    g = gy
    for l in reversed(range(nl)):
        if l < nl - 1:
            g = g * (z[l] > 0)
        dz[l] = g
        dW[l] = imatmul(g.T, acts[l])
        db[l] = g.sum(0)
        g = imatmul(g, W[l])
    h = dims[1] if nl > 1 else 0
    hidden = np.concatenate(acts[1:], 1) if nl > 1 else np.zeros((n, 0), np.int64)

    def f32(a):
        return None if a is None else torch.from_numpy(a.astype(np.float32))

    return dict(dims=dims, n=n, nl=nl, h=h, x=f32(x), grad_y=f32(gy), weights=[f32(w) for w in W],
                biases=[f32(b) for b in B], W=W, B=B, acts=acts, z=z, y=z[-1], hidden=hidden, dz=dz, grad_x=g, dW=dW, db=db,
                _cache={})


def hash_dims(dims):
    v = 17
    for d in dims:
        v = (v * 1000003 + d) % (2 ** 31)
    return v


@functools.lru_cache(maxsize=None)
def feature_case(h, n):
    """the feature head 48 -> h -> h -> 32 with the residual connection: the case above plus grad_geo0 [n] and the
    reference grad_geo [n, 33] = (grad_geo0 | grad_y + grad_x[:, :32])"""
    c = dict(case((48, h, h, 32), n, seed=1))
    rng = np.random.RandomState(n + h)
    col0 = rng.randint(-2, 3, size=(n,)).astype(np.int64)
    c["grad_geo0"] = torch.from_numpy(col0.astype(np.float32))
    c["grad_geo"] = np.concatenate([col0[:, None], c["grad_y"].numpy().astype(np.int64) + c["grad_x"][:, :32]], 1)
    return c


def largest_sums(c):
    """the largest S of each family of the module docstring -> dict"""
    if "sums" in c["_cache"]:
        return c["_cache"]["sums"]
    nl = c["nl"]
    aW = [np.abs(w) for w in c["W"]]
    out = dict(forward=0, data=0, weight=0, bias=0)
    for l in range(nl):
        a, d = np.abs(c["acts"][l]), np.abs(c["dz"][l])
        s = imatmul(a, aW[l].T)
        if c["B"][l] is not None:
            s = s + np.abs(c["B"][l])
        out["forward"] = max(out["forward"], int(s.max()))
        out["data"] = max(out["data"], int(imatmul(d, aW[l]).max()))
        out["weight"] = max(out["weight"], PREFILL + int(imatmul(d.T, a).max()))
        out["bias"] = max(out["bias"], PREFILL + int(d.sum(0).max()))
    if "grad_geo" in c:
        res = np.abs(c["grad_y"].numpy().astype(np.int64)) + imatmul(np.abs(c["dz"][0]), aW[0])[:, :32]
        out["data"] = max(out["data"], int(res.max()))
    c["_cache"]["sums"] = out
    return out


def assert_exact_operands(c):
    """every sum the kernels form, in any order, stays an fp32 integer: max S < 2^24 (see the module docstring)"""
    for k, v in largest_sums(c).items():
        assert v < LIMIT, f"{c['dims']} n={c['n']}: {k} sums of absolute products reach {v} >= 2^24"


def assert_informative(c):
    """every hidden layer has live and dead units on a quarter of its entries each and a pre-activation that is exactly 0;
    no reference output is all zero"""
    what = f"{c['dims']} n={c['n']}"
    for l in range(c["nl"] - 1):
        z = c["z"][l]
        live = float((z > 0).mean())
        assert 0.25 <= live <= 0.75, f"{what}: layer {l} has {live:.2f} of its units live"
        assert (z == 0).any(), f"{what}: layer {l} has no pre-activation that is exactly 0"
    outs = [("y", c["y"]), ("grad_x", c["grad_x"])] + [(f"dW[{l}]", a) for l, a in enumerate(c["dW"])] + \
           [(f"db[{l}]", a) for l, a in enumerate(c["db"])] + [(f"dz[{l}]", a) for l, a in enumerate(c["dz"])]
    if c["nl"] > 1:
        outs.append(("hidden", c["hidden"]))
    if "grad_geo" in c:
        outs.append(("grad_geo", c["grad_geo"]))
    for name, a in outs:
        assert a.any(), f"{what}: reference {name} is all zero"


def assert_equal(got, want, what):
    """bit for bit (as values: -0 == +0) against an int64 reference; names the first differing element"""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = np.asarray(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    assert np.abs(w).max(initial=0) < LIMIT, f"{what}: the reference itself is no fp32 integer"
    bad = ~(g == w.astype(g.dtype))  # a nan differs
    if bad.any():
        idx = tuple(int(k) for k in np.argwhere(bad)[0])
        where = f"row {idx[0]}, column {idx[1]}" if len(idx) == 2 else f"index {idx}"
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} elements differ; first at {where}: "
                             f"got {g[idx].item()!r}, want {int(w[idx])}")


# ---- the launch plans, restated ------------------------------------------------------------------------------------------
# mlp_chain.hip:611  #define NR_CHAIN_SHAPES(X)
#   X(32, 64, 33, 2) X(32, 32, 33, 2) X(48, 64, 32, 3) X(48, 32, 32, 3) X(64, 64, 32, 3) X(64, 32, 32, 3)
CHAINED = ((32, 64, 33), (32, 32, 33), (48, 64, 64, 32), (48, 32, 32, 32), (64, 64, 64, 32), (64, 32, 32, 32))


def _blocks(dims):
    """Shape<IN, H, OUT, NL>: `NB = H / 16, IB = IN / 16, OB = (OUT + 15) / 16, KP = OB * 16`"""
    return dims[1] // 16, dims[0] // 16, (dims[-1] + 15) // 16


def wg_mask(dims):
    """wg_mask(): `t0 = nb * ib, t1 = NL == 3 ? nb * nb : 0, tl = ob * nb; if (t0 + t1 + tl <= 24) return (1 << NL) - 1;
    if (t1 + tl <= 24) return ((1 << NL) - 1) & ~1; return 0;`"""
    nb, ib, ob = _blocks(dims)
    nl = len(dims) - 1
    t0, t1, tl = nb * ib, nb * nb if nl == 3 else 0, ob * nb
    if t0 + t1 + tl <= 24:
        return (1 << nl) - 1
    if t1 + tl <= 24:
        return ((1 << nl) - 1) & ~1
    return 0


def nslot(dims, mask=None):
    """WgShape: `NACC = AL + (LL ? OB * NB : 0)` accumulators of 4 floats after `A1 = A0 + (L0 ? NB * IB : 0)`,
    `AL = A1 + (L1 ? NB * NB : 0)`; `B0 = NACC * 4; B1 = B0 + (L0 ? NB * 4 : 0); BL = B1 + (L1 ? NB * 4 : 0);
    NSLOT = BL + (LL ? KS : 0)` with `KS = S::KP / 4`"""
    nb, ib, ob = _blocks(dims)
    nl = len(dims) - 1
    mask = wg_mask(dims) if mask is None else mask
    l0, l1, ll = bool(mask & 1), nl == 3 and bool(mask & 2), bool((mask >> (nl - 1)) & 1)
    nacc = l0 * nb * ib + l1 * nb * nb + ll * ob * nb
    return 4 * nacc + l0 * nb * 4 + l1 * nb * 4 + ll * (16 * ob // 4)


def part_floats(dims, mask=None):
    """`PART_FLOATS = NSLOT * 64`: one workgroup's partial; mlp_chain_part_floats() asks for 1024 of them"""
    return nslot(dims, mask) * 64


def mask_from_workspace(dims, n, floats):
    """the fused mask that nrhip_mlp_bwd_workspace's answer implies: answer - dZ block = NSLOT * 64 * 1024"""
    nl = len(dims) - 1
    extra = floats - ((n * (nl - 1) * dims[1] + 3) & ~3)
    full = (1 << nl) - 1
    hits = [m for m in (full, full & ~1, 0) if extra == part_floats(dims, m) * 1024]
    assert len(hits) == 1, (dims, n, floats, extra)
    return hits[0]


def pad4(v):
    return (v + 3) & ~3


def pad16(v):
    return (v + 15) & ~15


def act_ld(dims):
    """act_ld(): `k = pad16(k); return ((k + 31) / 32) * 32 + 2;` with k the widest of in, hidden, out"""
    widths = (dims[0], dims[-1]) + ((dims[1],) if len(dims) > 2 else ())
    return (pad16(max(widths)) + 31) // 32 * 32 + 2


def frag_floats(dims, l, transposed):
    """frag_floats(): `return pad16(rows) * pad4(k);` rows = out, k = in of layer l (forward) or the reverse (transposed)"""
    o, i = layer_dims(dims)[l]
    return pad16(i) * pad4(o) if transposed else pad16(o) * pad4(i)


def lds_bytes(dims, waves, transposed=False):
    """lds_bytes(): `return (w + (size_t)waves * 2 * 16 * act_ld(d)) * sizeof(float);`"""
    w = sum(frag_floats(dims, l, transposed) for l in range(len(dims) - 1))
    return (w + waves * 2 * 16 * act_ld(dims)) * 4


def pick_waves(dims, transposed=False):
    """pick_waves(): `for (int w = 4; w >= 1; w >>= 1) if (lds_bytes<TRANSPOSED>(d, w) <= 160 * 1024) return w; return 0;`"""
    for w in (4, 2, 1):
        if lds_bytes(dims, w, transposed) <= 160 * 1024:
            return w
    return 0


def blocks_for_tiles(n, waves):
    """blocks_for_tiles(): `b = (tiles + waves - 1) / waves; if (b > 2048) b = 2048; if (b < 1) b = 1;`"""
    tiles = (n + 15) // 16
    return max(1, min(2048, (tiles + waves - 1) // waves))


def wgrad_grid(dims, n, layers=None):
    """run_wgrad(): `bx = ((n + 3) / 4 + 4 * 64 - 1) / (4 * 64); if (bx > 256) bx = 256; if (bx < 1) bx = 1;` and
    `nsub += ((out + 63) / 64) * L.nb_in` with `L.nb_in = (in + 63) / 64` over the layers it serves -> (bx, nsub, [sub0])"""
    shapes = layer_dims(dims)
    layers = range(len(shapes)) if layers is None else layers
    bx = max(1, min(256, ((n + 3) // 4 + 255) // 256))
    nsub, sub0 = 0, []
    for l in layers:
        o, i = shapes[l]
        sub0.append(nsub)
        nsub += ((o + 63) // 64) * ((i + 63) // 64)
    return bx, nsub, sub0


def chain_workgroups(n, cap):
    """grid_blocks(): `want = ((n + 15) / 16 + 3) / 4; cap = (int64_t)cu_count() * per_cu; return want < cap ? (want < 1 ? 1
    : want) : cap;`; launch_bwd_wg(): `if (blocks > fit) blocks = (int)fit;` -- `cap` is the smaller of the two"""
    want = ((n + 15) // 16 + 3) // 4
    return max(1, want) if want < cap else cap


# ---- the cases of tests/test_gpu_mlp_exact.py (tests/test_mlp_refs_host.py checks every one on the CPU) ----------------------
CHAIN_NS = (1, 15, 16, 17, 1000, 70001)    # 70001: 1094 workgroups' worth of tiles > cu_count * 4 on any part
SWITCH_NS = (17, 1000)
DEEP = (20,) * 9                            # NRHIP_MAX_LAYERS = 8 layers of width 20
GENERIC = (                                 # (dims, keywords of case())
    ((3, 7, 5), {"seed": 1}),
    ((13, 24, 24, 24, 3), {"no_bias": (0, 2)}),
    ((5, 100, 9), {}),
    ((200, 7), {}),
    ((70, 130, 65), {}),
    (DEEP, {"gain": 4.0, "no_bias": (1, 3, 5, 7), "seed": 4}),  # (the seeds: the first for which assert_informative holds at every n)
)
GENERIC_NS = (1, 17, 100)                   # 100 rows: 7 tiles, two workgroups of 4 waves
TWO_WAVES, ONE_WAVE, TOO_LARGE = (48, 128, 128, 16), (64, 144, 144, 16), (256, 256, 256, 256)
PLAN_NS = (17, 100)
FWD_CAPPED = ((3, 5, 2), 131089)            # 8194 tiles > 2048 workgroups x 4 waves
WGRAD_RAGGED, WGRAD_NS = (70, 130, 65), (1, 2, 3, 5, 1023)
WGRAD_CAPPED = ((5, 7, 3), 262149)          # 65,538 sample quads: 257 slices asked, 256 launched
MERGE_COUNTS = (1, 3, 4, 5, 13, 16, 17, 29)
MERGE_SHAPES = ((32, 32, 33), (48, 64, 64, 32))  # a full and a partial mask
FEATURE_NS = (1, 15, 17, 1000, 70001)
SINGLE = (9, 6)                             # one layer: no data kernel unless grad_x is asked for


def gpu_cases():
    """every (dims, n, keywords) that the GPU module builds with case(); feature_case(h, n) for h in (32, 64), n in FEATURE_NS
    comes on top"""
    out = [(d, n, {}) for d in CHAINED for n in CHAIN_NS]
    out += [(d, n, kw) for d, kw in GENERIC for n in GENERIC_NS]
    out += [(d, n, {}) for d in (TWO_WAVES, ONE_WAVE) for n in PLAN_NS]
    out += [FWD_CAPPED + ({},), WGRAD_CAPPED + ({},)]
    out += [(WGRAD_RAGGED, n, {}) for n in WGRAD_NS]
    out += [(d, 64 * k - 7, {}) for d in MERGE_SHAPES for k in MERGE_COUNTS]
    out += [(SINGLE, n, {}) for n in GENERIC_NS]
    seen, uniq = set(), []
    for d, n, kw in out:
        key = (d, n, tuple(sorted(kw.items())))
        if key not in seen:
            seen.add(key), uniq.append((d, n, kw))
    return uniq
