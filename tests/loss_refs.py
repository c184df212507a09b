"""References and case builders of the loss kernels: lidar_carving_kernel, interlevel_loss_kernel and
distortion_loss_kernel (csrc/losses.hip), mask_compact_kernel, lidar_rays_kernel, lidar_finish_kernel and
lidar_losses_bwd_kernel (csrc/train_fused.hip).  tests/test_loss_refs_host.py checks this module on the CPU,
tests/test_gpu_loss_kernels.py compares the kernels with it.  Everything here is CPU torch / numpy.

WHAT IS EXACT AND WHY.
  carving    edges are multiples of 1/64 below 256, distances multiples of 1/128, eps = 1/8, non_return = 128: every
             midpoint (a + b) * 0.5 and every difference d - mid is a multiple of 1/128 below 512, exact in fp32 whatever
             the order of the operations.  The mask is a comparison of exact numbers: torch.equal.  2 * w is exact.
  lidar err  |where(ret, dist, max(pred, nr)) - pred| (* nr_mult) is one subtraction and at most one multiplication, each
             rounded once, the same in torch fp32 and in the kernel: bit equality.  With pred = 0 and did_return = True the
             error IS the distance, so any non-negative bit pattern can be put in front of the select.
  threshold  torch.quantile(err, q) on the CPU.  `radix_threshold` restates the kernel's arithmetic (fp32 rank, four 8-bit
             passes, the count of values <= the low order statistic, the smallest value above it, at::lerp's two-sided
             form) and the host test demands bit equality of the two on every quantile case, which makes bit equality a
             fair demand on the kernel.
  kept set   err < thr on exact numbers; the counts are integers below 2^24, exact in fp32.
Gradients outside the kept set are DEFINED as zero (the kernel's `err < thr ? g / count : 0`), also when the kept set is
empty: torch autograd would give 0 * inf there, but the metric itself is already 0 / 0.

WRONG VARIANTS.  `variant=` builds the expected output of a kernel with one plausible mistake; the host test demands that
every variant changes the expected output of at least one GPU case (CARVING_VARIANTS, LIDAR_VARIANTS).  All of them are
told apart by the case lists below; none had to be given up."""
import functools

import numpy as np
import torch

f32 = np.float32

CARVING_VARIANTS = ("eps_le", "nr_le", "swap")
LIDAR_VARIANTS = ("keep_le", "vhi_is_vlo", "rank_fp64", "lerp_one_sided", "swap", "max_is_nr")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- lidar_carving ---------------------------------------------------------------------------------------------------------
EPS = 0.125
NON_RETURN = 128.0
# every value of R and S of the issue; R % 4 != 0 with S > 64: (1, 129), (3, 65), (5, 129), (1027, 65)
CARVING_SHAPES = ((1, 129), (3, 65), (4, 64), (5, 129), (1027, 65), (4, 1), (5, 63), (1027, 1), (3, 63))


def carving_ref(starts, ends, is_lidar, did_return, distance, eps, non_return, weights=None, variant=None):
    """-> (is_close [R,S] bool, loss per ray [R] fp64 or None, d loss / d weights [R,S] fp64 or None).  The mask in torch
    fp32 is the reference's _compute_is_close_to_lidar (models/neurad.py:677-700); did_return=None: all returned."""
    mid = (starts + ends) * 0.5
    R = mid.shape[0]
    ret = torch.ones(R, dtype=torch.bool) if did_return is None else did_return.reshape(-1).bool()
    if variant == "swap":
        ret = ~ret
    dist = (distance.reshape(-1, 1) - mid).abs()
    hit = dist <= eps if variant == "eps_le" else dist < eps
    in_range = mid <= non_return if variant == "nr_le" else mid < non_return
    lidar = is_lidar.reshape(-1, 1).bool()
    close = torch.where(ret[:, None], hit, in_range) & lidar
    if weights is None:
        return close, None, None
    far = (lidar & ~close).double()
    wf = weights.double() * far
    return close, wf.square().sum(-1), 2.0 * wf


@functools.lru_cache(maxsize=None)
def carving_case(R, S, seed=0, extra=3):
    """Edges [R, S + 1 + extra] (the kernel sees a row stride of S + 1 + extra), per-ray is_lidar / did_return / distance,
    weights [R,S].  Rays 0, 3, 6, ... are planted on a band edge: a returned one gets distance = mid[s] +- eps for one of
    its samples (|d - mid| == eps: NOT close), a non-returned one gets a bin whose midpoint is exactly non_return (NOT in
    range).  Rays 0 and 1 are lidar rays; ray 0 has returned, ray 1 has not.  `share` = (samples with |d - mid| == eps on
    returned lidar rays, samples with mid == non_return on the other lidar rays) / all lidar samples.  One planted sample
    per third ray is about 1 / (3 S): over CARVING_SHAPES the first share is 1.9e-3 (R = 5, S = 129) .. 0.25 (R = 4, S = 1),
    the second 1.9e-3 .. 0.5, and 0 only at R = 1, whose single ray has returned."""
    g = _gen(1000 * R + S + seed)
    W = S + 1 + extra
    nr64 = int(NON_RETURN * 64)
    e = torch.sort(torch.randint(0, 256 * 64, (R, W), generator=g), -1).values
    is_lidar = torch.rand(R, generator=g) < 0.7
    ret = torch.rand(R, generator=g) < 0.6
    is_lidar[:2] = True
    ret[0] = True
    if R > 1:
        ret[1] = False
    planted = torch.zeros(R, dtype=torch.bool)
    planted[0::3] = True
    if R > 1:
        planted[1] = True
    for r in torch.nonzero(planted & ~ret).reshape(-1).tolist():  # a bin centred on non_return
        s = int(torch.randint(0, S, (1,), generator=g))
        a = int(torch.randint(0, 65, (1,), generator=g))  # a == 0: a zero-width bin on the edge itself
        lo = torch.sort(torch.randint(0, nr64 - a + 1, (s + 1,), generator=g)).values
        hi = torch.sort(torch.randint(nr64 + a, 256 * 64, (W - s - 1,), generator=g)).values
        lo[-1], hi[0] = nr64 - a, nr64 + a
        e[r] = torch.cat([lo, hi])
    edges = e.float() / 64.0
    mid = (edges[:, :S] + edges[:, 1:S + 1]) * 0.5
    dist = torch.randint(0, 256 * 128, (R,), generator=g).float() / 128.0
    rows = torch.nonzero(planted & ret).reshape(-1)
    s = torch.randint(0, S, (rows.numel(),), generator=g)
    sign = torch.where(torch.arange(rows.numel()) % 2 == 0, 1.0, -1.0)
    dist[rows] = mid[rows, s] + sign * EPS
    weights = torch.rand(R, S, generator=g)
    assert float(edges.max()) < 256 and torch.equal(edges * 64, (edges * 64).round())
    c = {"R": R, "S": S, "edges": edges, "is_lidar": is_lidar, "did_return": ret, "distance": dist, "weights": weights}
    c["share"] = carving_share(c, is_lidar, ret)
    return c


def carving_share(c, is_lidar, did_return):
    """share of the lidar samples that sit exactly on |d - mid| == eps (returned) or mid == non_return (not returned)"""
    S = c["S"]
    mid = (c["edges"][:, :S] + c["edges"][:, 1:S + 1]) * 0.5
    on_eps = ((c["distance"][:, None] - mid).abs() == EPS) & (is_lidar & did_return)[:, None]
    on_nr = (mid == NON_RETURN) & (is_lidar & ~did_return)[:, None]
    n = max(int(is_lidar.sum()) * S, 1)
    return int(on_eps.sum()) / n, int(on_nr.sum()) / n


# ---- torch.quantile as the kernel computes it -------------------------------------------------------------------------------
def radix_threshold(err, q, variant=None):
    """lidar_finish_kernel's select on the non-negative fp32 array `err`: -> the threshold as np.float32"""
    err = np.ascontiguousarray(err, f32)
    u = err.view(np.uint32)
    n = u.size
    if variant == "rank_fp64":
        rank64 = float(f32(q)) * (n - 1)
        k_lo, k_hi = int(rank64), int(np.ceil(rank64))
        wq = f32(rank64 - k_lo)
    else:
        rank = f32(q) * f32(n - 1)  # fp32, as `q * last_index` on a float32 tensor
        k_lo, k_hi = int(rank), int(np.ceil(rank))
        wq = rank - f32(k_lo)
    prefix, k = 0, k_lo
    for p in range(4):  # four 8-bit passes over the bit patterns, most significant byte first
        shift = 24 - 8 * p
        himask = 0 if p == 0 else (0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF
        sel = u[(u & np.uint32(himask)) == np.uint32(prefix)]
        hist = np.bincount(((sel >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, k, side="right"))
        k -= int(cum[b] - hist[b])
        prefix |= b << shift
    cle = int((u <= np.uint32(prefix)).sum())  # values <= the low order statistic
    above = u[u > np.uint32(prefix)]
    v_lo = np.array([prefix], np.uint32).view(f32)[0]
    if k_hi == k_lo or cle > k_hi or above.size == 0 or variant == "vhi_is_vlo":
        v_hi = v_lo
    else:
        v_hi = np.array([above.min()], np.uint32).view(f32)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        if wq < f32(0.5) or variant == "lerp_one_sided":  # at::lerp
            return f32(v_lo + wq * (v_hi - v_lo))
        return f32(v_hi - (v_hi - v_lo) * (f32(1) - wq))


def bits(a):
    """fp32 array or tensor -> its bit patterns (int32 numpy)"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.int32)


# ---- lidar losses -------------------------------------------------------------------------------------------------------
NR_DIST, NR_MULT = 150.0, 0.1
UPSTREAM = (1.0, 0.7, 1.3, 0.9, 1.1, 0.6)


def lidar_case(n, seed=0, levels=3, q=0.95, err=None, ret=None, pred0=None, plant=True):
    """One batch of R = 2 n + 3 rays with n lidar rays scattered among them.  Depth levels are drawn in [1, 200] against
    non_return_lidar_distance = 150, so `fmaxf(pred, nr_dist)` takes both sides; with n >= 8 and plant, the first lidar rays
    are (1) not returned with pred == nr_dist, (2) not returned and beyond it, (3) not returned and short of it,
    (4) returned with pred == distance, on every level.  err (fp32 [n], non-negative): the field level predicts 0 and every
    beam returns, so the error vector is `err` exactly.  ret / pred0: did_return [n] / the field level's prediction at the
    lidar rays [n] as given."""
    g = _gen(7919 * n + seed)
    R = 2 * n + 3
    is_lidar = torch.zeros(R, dtype=torch.bool)
    is_lidar[torch.randperm(R, generator=g)[:n]] = True
    rows = torch.nonzero(is_lidar).reshape(-1)
    did = torch.rand(n, generator=g) < 0.8
    dist = torch.rand(n, generator=g) * 78 + 2
    depths = [torch.rand(R, generator=g) * 199 + 1 for _ in range(levels)]
    if plant and n >= 8:
        did[1:4], did[4] = False, True
        for d in depths:
            d[rows[1]], d[rows[2]], d[rows[3]], d[rows[4]] = NR_DIST, NR_DIST + 25.0, NR_DIST - 25.0, dist[4]
    if ret is not None:
        did = ret.clone()
    if pred0 is not None:
        depths[0][rows] = pred0
    if err is not None:
        e = torch.from_numpy(np.ascontiguousarray(err, f32))
        assert e.shape == (n,) and bool((bits(e) >= 0).all())
        did = torch.ones(n, dtype=torch.bool)
        dist = e.clone()
        depths[0][rows] = 0.0
    return {"n": n, "R": R, "levels": levels, "q": q, "is_lidar": is_lidar, "rows": rows, "did_return": did,
            "distance": dist, "depths": depths, "intensity": torch.rand(n, generator=g),
            "target": torch.rand(n, generator=g), "logits": torch.randn(n, generator=g),
            "up": torch.tensor(UPSTREAM[:2 + levels]), "nr_dist": NR_DIST, "nr_mult": NR_MULT}


def _level_err(pred, dist, ret, nr, mult, variant=None):
    """per-ray |target - pred| (x nr_mult without a return) in the dtype of `pred`, and d err / d pred"""
    if variant == "swap":
        ret = ~ret
    beyond = torch.full_like(pred, nr) if variant == "max_is_nr" else pred.clamp_min(nr)
    diff = torch.where(ret, dist.to(pred.dtype), beyond) - pred
    m = torch.where(ret, torch.ones_like(pred), torch.full_like(pred, float(f32(mult)) if pred.dtype == torch.float64 else mult))
    return diff.abs() * m, -torch.sign(diff) * m


def lidar_ref(c, variant=None):
    """-> err (fp32 [n]), thr (fp32 0-dim, torch.quantile on the CPU), keep (bool [n]), n_keep, n_sel, metrics (fp64
    [2 + levels]: depth_loss, intensity_loss, ray_drop_loss, depth_loss_0, ...), and per element in fp64 for the upstream
    gradients c["up"]: gdepth (levels x [R]), gint [n], glogit [n].  A variant changes the expected output as a kernel
    with that mistake would (its threshold then comes from radix_threshold)."""
    n, R, nl, rows, ret = c["n"], c["R"], c["levels"], c["rows"], c["did_return"]
    err, _ = _level_err(c["depths"][0][rows], c["distance"], ret, c["nr_dist"], c["nr_mult"], variant)
    if variant is None:
        thr = torch.quantile(err, c["q"])
    else:
        thr = torch.tensor(radix_threshold(err.numpy(), c["q"], variant))
    keep = err <= thr if variant == "keep_le" else err < thr
    sel = keep & ret
    n_keep, n_sel = int(keep.sum()), int(sel.sum())
    up = c["up"].double()
    metrics = torch.full((2 + nl,), float("nan"), dtype=torch.float64)
    gdepth = [torch.zeros(R, dtype=torch.float64) for _ in range(nl)]
    with np.errstate(all="ignore"):
        e64, dp64 = _level_err(c["depths"][0][rows].double(), c["distance"], ret, c["nr_dist"], c["nr_mult"], variant)
        metrics[0] = e64[keep].sum() / n_keep if n_keep else float("nan")
        if n_keep:
            gdepth[0][rows] = torch.where(keep, dp64 * up[0] / n_keep, torch.zeros_like(dp64))
        di = c["target"].double() - c["intensity"].double()
        metrics[1] = di[sel].square().sum() / n_sel if n_sel else float("nan")
        gint = torch.where(sel, -2.0 * di / n_sel * up[1], torch.zeros_like(di)) if n_sel else torch.zeros_like(di)
        x, y = c["logits"].double(), (~ret).double()
        metrics[2] = (x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
        glogit = (torch.sigmoid(x) - y) / n * up[2]
        for l in range(1, nl):
            el, dl = _level_err(c["depths"][l][rows].double(), c["distance"], ret, c["nr_dist"], c["nr_mult"], variant)
            metrics[2 + l] = el.mean()
            gdepth[l][rows] = dl / n * up[2 + l]
    return {"err": err, "thr": thr, "keep": keep, "n_keep": n_keep, "n_sel": n_sel, "metrics": metrics, "gdepth": gdepth,
            "gint": gint, "glogit": glogit}


def _from_bits(u):
    return np.asarray(u, np.uint32).view(f32)


def byte_errors(k, n=300, seed=0):
    """n errors whose bit patterns differ only in byte k (0 = least significant) of 0x3F9A5C33: pass 3 - k of the select
    decides alone.  Byte 3 stays below 0x80 (the sign) and is kept off 0x7F with a non-zero mantissa (NaN)."""
    rs = np.random.RandomState(100 + k + seed)
    base = 0x3F9A5C33 & ~(0xFF << (8 * k)) & 0xFFFFFFFF
    b = rs.randint(0, 0x7F if k == 3 else 256, n).astype(np.uint32)
    return _from_bits(np.uint32(base) | (b << np.uint32(8 * k)))


def mixed_errors(n=300, n_inf=4, seed=0):
    """0, denormals, ordinary values and +inf"""
    rs = np.random.RandomState(200 + seed)
    e = rs.uniform(0.0, 80.0, n).astype(f32)
    e[0:40] = 0.0
    e[40:120] = _from_bits(rs.randint(1, 0x00800000, 80).astype(np.uint32))  # denormals
    e[120:120 + n_inf] = np.inf
    return e[rs.permutation(n)]


def tie_errors(kind, n, q=0.95):
    """ties around the two order statistics of rank q (n - 1)"""
    rank = f32(q) * f32(n - 1)
    k_lo, k_hi = int(rank), int(np.ceil(rank))
    if k_hi == k_lo:  # (n = 21: the fp32 rank 0.95f * 20 is 19 exactly) the statistic and its upper neighbour
        k_lo, k_hi = k_lo - 1, k_lo
    e = np.sort(np.random.RandomState(300 + n).uniform(1.0, 50.0, n).astype(f32))
    if kind == "all_equal":
        e[:] = 7.25
    elif kind == "both_equal":  # v_lo == v_hi with more copies below and above
        e[k_lo - 2:min(k_hi + 2, n)] = e[k_lo]
    elif kind == "lo_dup":  # the low statistic three times, a distinct high one
        e[k_lo - 2:k_lo + 1] = e[k_lo]
    elif kind == "hi_dup":  # the high statistic to the end of the array
        e[k_hi:] = e[k_hi]
    else:
        raise ValueError(kind)
    return e[np.random.RandomState(n).permutation(n)]


def lerp_errors(n=10, q=0.95):
    """errors whose two order statistics make at::lerp's second form (weight >= 0.5: b - (b - a)(1 - w)) round differently
    from the one-sided a + w (b - a): found by drawing until the two differ (about one draw in ten does)"""
    rs = np.random.RandomState(400 + n)
    for _ in range(1000):
        e = rs.uniform(1.0, 50.0, n).astype(f32)
        if radix_threshold(e, q) != radix_threshold(e, q, "lerp_one_sided"):
            return e
    raise AssertionError("no draw separates the two forms of lerp")


SIZE_NS = (1, 2, 255, 256, 257, 16385, 32768, 32769, 40000)
TIE_KINDS = ("all_equal", "both_equal", "lo_dup", "hi_dup")


@functools.lru_cache(maxsize=None)
def lidar_cases():
    """name -> case: every lidar case of tests/test_gpu_loss_kernels.py (built once, never modified)"""
    cs = {}
    # lidar_rays_kernel: one 256-ray workgroup / two; lidar_finish_kernel: dynamic LDS past 64 KB (n > 16384), the LDS
    # limit `n <= kLossLds` (32768), and the branch that reads the errors back from memory (32769, 40000)
    for n in SIZE_NS:
        cs[f"size_{n}"] = lidar_case(n)
    # lidar_finish_kernel's radix passes: `(u & himask) == prefix`, `(u >> shift) & 255`
    for k in range(4):
        cs[f"byte_{k}"] = lidar_case(300, err=byte_errors(k))
    cs["mixed_inf"] = lidar_case(300, err=mixed_errors())                # 0, denormals, +inf; v_hi finite
    cs["mixed_inf_hi"] = lidar_case(300, err=mixed_errors(n_inf=15))     # v_hi = +inf: everything finite is kept
    # `(int64_t)s_cle > k_hi` and `s_mgt`: v_hi with duplicates of v_lo
    for n in (21, 41):
        for kind in TIE_KINDS:
            cs[f"tie_{kind}_{n}"] = lidar_case(n, err=tie_errors(kind, n))
    # `rank`, `k_hi == k_lo`, `wq < 0.5f`
    for q in (0.0, 1.0, 0.5):
        cs[f"q_{q}"] = lidar_case(300, q=q)
    for n, q in ((9, 0.95), (11, 0.95), (300, 0.999)):  # wq = 0.6, 0.5, 0.7: at::lerp's second form
        cs[f"lerp_hi_{n}"] = lidar_case(n, q=q, seed=4)
    cs["lerp_forms_differ"] = lidar_case(10, err=lerp_errors())  # wq = 0.55, and the one-sided form is one ulp away
    cs["q_0.5_even"] = lidar_case(301, q=0.5)      # rank 150 exactly
    cs["rank_integral"] = lidar_case(21, q=0.95)   # 0.95f * 20 rounds to 19 in fp32 (18.9999998 in fp64)
    # depth_l1: `fmaxf(pred, nr_dist)` on both sides and at equality, `diff == 0`
    n = 64
    ret = torch.arange(n) % 2 == 0
    c0 = lidar_case(n, seed=1, ret=ret, plant=False)
    pred = c0["depths"][0][c0["rows"]].clone()
    pred[1::6], pred[3::6], pred[5::6] = NR_DIST - 30.0, NR_DIST, NR_DIST + 30.0   # not returned: below, equal, above
    pred[0::4] = c0["distance"][0::4]                                              # returned: pred == distance
    cs["branches"] = lidar_case(n, seed=1, ret=ret, pred0=pred, plant=False)
    cs["none_returned"] = lidar_case(64, seed=2, ret=torch.zeros(64, dtype=torch.bool), plant=False)  # intensity: 0 / 0
    # kMaxDepthLevels: `if (l >= A.n_levels) break`
    for nl in (1, 2, 4):
        cs[f"levels_{nl}"] = lidar_case(300, seed=3, levels=nl)
    return cs


def lidar_metrics_cpu(c, up=None):
    """lidar_metrics(fused=False) of the package on the CPU with autograd: -> (metrics fp32 [2 + levels], gradients of
    sum(up * metrics): depth levels [R] each, intensity [n], logits [n])"""
    from neurad_studio_amd.model_components.lidar_losses import LidarLossSettings, lidar_metrics

    nl = c["levels"]
    cfg = LidarLossSettings(quantile_threshold=c["q"], non_return_lidar_distance=c["nr_dist"],
                            non_return_loss_mult=c["nr_mult"])
    d = [t.clone()[:, None].requires_grad_(True) for t in c["depths"]]
    i, lg = c["intensity"].clone()[:, None].requires_grad_(True), c["logits"].clone()[:, None].requires_grad_(True)
    out = {"depth": d[0], "intensity": i, "ray_drop_logits": lg, "non_nearby_weights_loss": torch.tensor(0.0)}
    for k in range(nl - 1):
        out[f"prop_depth_{k}"], out[f"prop_weights_loss_{k}"] = d[k + 1], torch.tensor(0.0)
    m = lidar_metrics(out, c["is_lidar"], c["did_return"], c["distance"][:, None], c["target"][:, None], cfg,
                      num_proposal_rounds=nl - 1, fused=False)
    names = ["depth_loss", "intensity_loss", "ray_drop_loss"] + [f"depth_loss_{k}" for k in range(nl - 1)]
    vals = torch.stack([m[k] for k in names])
    (vals * (c["up"] if up is None else up)).sum().backward()
    return vals.detach(), [t.grad[:, 0] for t in d], i.grad[:, 0], lg.grad[:, 0]


# ---- mask_compact -------------------------------------------------------------------------------------------------------
MASK_RS = (0, 1, 7, 8, 9, 8191, 8192, 8193, 8200, 16389)
MASK_OFFSETS = (1, 3, 7)  # bytes off an 8-byte boundary: mask_compact_kernel's `aligned` is false, byte loads


def mask_cases(R):
    """name -> bool mask [R]: densities 0 / 0.5 / 1, only the last element, only the two elements either side of every
    8192-ray pass boundary"""
    g = _gen(R)
    last, edge = torch.zeros(R, dtype=torch.bool), torch.zeros(R, dtype=torch.bool)
    last[-1:] = True
    for b in range(8192, R + 1, 8192):
        edge[b - 1] = True
        if b < R:
            edge[b] = True
    return {"zeros": torch.zeros(R, dtype=torch.bool), "half": torch.rand(R, generator=g) < 0.5,
            "ones": torch.ones(R, dtype=torch.bool), "last": last, "pass_edges": edge}


def compact_ref(mask):
    """-> (rows int64 [count], inverse int32 [R]) of a CPU mask of any dtype"""
    m = mask.reshape(-1) != 0
    rows = torch.nonzero(m).reshape(-1)
    inv = torch.full((m.numel(),), -1, dtype=torch.int32)
    inv[rows] = torch.arange(rows.numel(), dtype=torch.int32)
    return rows, inv


# ---- interlevel / distortion ------------------------------------------------------------------------------------------------
# (R, sf, sp): every value of the issue.  scan_inplace runs over M - 1 = 2 sf + 1 knots in chunks of 64 lanes: 63 / 65 / 67
# at sf = 31 / 32 / 33, 129 at 64, 257 at 128; the proposal edges are sp + 1 = 64 / 65 / 66 at sp = 63 / 64 / 65, 129, 513.
# R = 5 and 9 leave one ray in the last 4-ray workgroup, R = 1 three idle waves.
SAMPLER_SHAPES = ((1, 1, 1), (4, 31, 63), (5, 32, 64), (9, 33, 65), (5, 64, 128), (9, 128, 512), (4, 32, 63), (1, 31, 65),
                  (5, 1, 512), (4, 128, 1))
PULSE = 0.03


@functools.lru_cache(maxsize=None)
def sampler_case(R, sf, sp, seed=0, zero_wp=False):
    """Fine edges / weights c [R, sf+1], w [R, sf] and proposal ones cp [R, sp+1], wp [R, sp] (numpy fp32) in [0, 1].
    Proposal edges 2, 3 (and every 7th after) are the fp32 values c[k] - r / c[k] + r of fine knots, so they EQUAL a knot
    of the blurred histogram and `L.x[mid] < x` (searchsorted's left rule) decides the bin; with sp >= 8 proposal bin 5 has
    zero width, and with sf >= 4 as well the fine bin 1 is 2^-12 wide with the zero-width proposal bin inside it.  (A fine bin
    of no width at all makes w / width infinite and the reference's loss NaN: `degenerate_sampler_case`.)"""
    rs = np.random.RandomState(10007 * R + 101 * sf + sp + seed)
    c = np.sort(rs.uniform(0.0, 1.0, (R, sf + 1)).astype(f32), -1)
    c[:, 0], c[:, -1] = 0.0, 1.0
    if sf >= 4:
        c[:, 2] = c[:, 1] + f32(2.0 ** -12)
        c = np.sort(c, -1)
    cp = np.sort(rs.uniform(0.0, 1.0, (R, sp + 1)).astype(f32), -1)
    cp[:, 0], cp[:, -1] = 0.0, 1.0
    if sp >= 8:
        r = f32(PULSE)
        for j in range(2, sp, 7):
            k = rs.randint(0, sf + 1, R)
            knot = c[np.arange(R), k] + (r if j % 2 else -r)
            cp[:, j] = np.where((knot > 0) & (knot < 1), knot, cp[:, j])
        if sf >= 4:
            cp[:, 5] = cp[:, 6] = c[:, 1] + f32(2.0 ** -13)
        cp = np.sort(cp, -1)
        if sf < 4:
            cp[:, 5] = cp[:, 6]
    w = rs.uniform(0.0, 1.0, (R, sf)).astype(f32)
    w = (w / w.sum(-1, keepdims=True) * f32(0.8)).astype(f32)
    wp = rs.uniform(0.2 / sp, 2.0 / sp, (R, sp)).astype(f32)
    if sp == 1:
        wp[:] = 0.3  # below the single bin's share of the fine histogram: a loss that is not 0
    if zero_wp:
        wp[:, 0] = 0.0
    return c, w, cp, wp


def degenerate_sampler_case(R=5, sf=32, sp=64):
    """sampler_case with fine bin 1 of ray 0 given no width at all, next to that ray's zero-width proposal bin: w / 0 is
    infinite, the blurred histogram holds inf - inf, and the reference's loss of that ray is NaN (torch's clamp_min and
    sum keep a NaN).  The other rays are ordinary."""
    c, w, cp, wp = (a.copy() for a in sampler_case(R, sf, sp))
    c[0, 2] = c[0, 1]
    cp[0, 5] = cp[0, 6] = c[0, 1]
    cp[0] = np.sort(cp[0])
    assert (np.diff(c, axis=-1) >= 0).all() and (np.diff(cp, axis=-1) >= 0).all()
    return c, w, cp, wp


def interlevel_ref64(c, w, cp, wp, r):
    """neurad_oracle.interlevel_loss_level's formula in float64 on fp32 inputs: -> loss [R], d loss / d wp [R, sp]"""
    c, w, cp, wp = (np.asarray(a, f32).astype(np.float64) for a in (c, w, cp, wp))
    r = float(f32(r))
    R = c.shape[0]
    loss, grad = np.zeros(R), np.zeros_like(wp)
    for i in range(R):
        wi = w[i].copy()
        wi[-1] += 1.0 - w[i].sum()
        wn = wi / (c[i, 1:] - c[i, :-1])
        xa = np.concatenate([c[i] - r, c[i] + r])
        idx = np.argsort(xa, kind="stable")
        xr = xa[idx]
        y1 = (np.concatenate([wn, [0.0]]) - np.concatenate([[0.0], wn])) / (2 * r)
        y2 = np.concatenate([y1, -y1])[idx[:-1]]
        yr = np.concatenate([[0.0], np.maximum(np.cumsum((xr[1:] - xr[:-1]) * np.cumsum(y2)), 0.0)])
        cdf = np.concatenate([[0.0, 0.0], np.cumsum(0.5 * (yr[1:] + yr[:-1]) * (xr[1:] - xr[:-1])), [1.0]])
        x_ = np.concatenate([[0.0], xr, [1.0]])
        y_ = np.concatenate([[0.0], yr, [0.0]])
        right = np.searchsorted(x_, cp[i], side="left")
        left = np.maximum(right - 1, 0)
        right = np.minimum(right, x_.size - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            off = (cp[i] - x_[left]) / (x_[right] - x_[left])
        off = np.clip(np.nan_to_num(off, nan=0.0), 0, 1)
        v = cdf[left] + (cp[i] - x_[left]) * (y_[left] + y_[right] * off + y_[left] * (1 - off)) * 0.5
        d = np.maximum(np.diff(v) - wp[i], 0.0)
        den = wp[i] + float(f32(1e-5))
        loss[i] = (d * d / den).sum()
        grad[i] = -(2 * d / den + d * d / (den * den))
    return loss, grad
