"""CPU restatement (numpy) of the occupancy-grid update rule, invisible-cell marking and the multi-level march of
csrc/occgrid_update.h / csrc/occgrid.hip -- TEST INFRASTRUCTURE ONLY, written from the rule's text, not from the kernels.

The rule is modelled on nerfacc 0.5 (OccGridEstimator._update / mark_invisible_cells / sampling).  nerfacc is un-vendored and
on no machine this was written on: PARITY WITH NERFACC ITSELF IS UNPINNED, exactly like the march (row S6).  What is pinned
is this statement.  Every function works in fp32 -- the kernels' arithmetic, operation for operation -- and, where a
discrete decision hangs on a comparison, also in float64, so that a test can leave out the cases the rounding decides."""
import numpy as np

f32, f64 = np.float32, np.float64


def level_aabbs(roi_aabb, levels):
    """[L,6] fp32: level l is the level-0 box scaled by 2^l about its centre"""
    a = np.asarray(roi_aabb, f32).reshape(6)
    centre, half = (a[:3] + a[3:]) * f32(0.5), (a[3:] - a[:3]) * f32(0.5)
    return np.stack([np.concatenate([centre - half * f32(2 ** l), centre + half * f32(2 ** l)]) for l in range(levels)])


def capacity(res, warmup, n=None):
    n = res ** 3 // 4 if n is None else n
    return n, (res ** 3 if warmup else 2 * n)


def shell_occ(x):
    """the quantised shell of the threshold check: floor(clip(1.5 - |x|, 0, 1) * 8) / 256"""
    x = np.asarray(x, f64)
    r = np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])
    return (np.floor(np.clip(1.5 - r, 0.0, 1.0) * 8.0) / 256.0).astype(f32)


def draws(res, levels, warmup, seed, n=None):
    """the three injected tensors of one update: cell_draws int64 [L,n], sel_draws fp32 [L,n], jitter fp32 [L,cap,3]"""
    rng = np.random.default_rng(seed)
    n, cap = capacity(res, warmup, n)
    return dict(cell_draws=rng.integers(0, res ** 3, (levels, n)), sel_draws=rng.random((levels, n), dtype=f32),
                jitter=rng.random((levels, cap, 3), dtype=f32))


# ---- candidates ------------------------------------------------------------------------------------------------------------
def candidates(occs, binaries, res, levels, warmup, n=None, cell_draws=None, sel_draws=None):
    """-> cell_ids int32 [L,cap] (-1 behind the count), counts int32 [L]"""
    cells = res ** 3
    n, cap = capacity(res, warmup, n)
    occs = np.asarray(occs, f32).reshape(levels, cells)
    binaries = np.asarray(binaries).reshape(levels, cells).astype(bool)
    ids = np.full((levels, cap), -1, np.int32)
    counts = np.zeros(levels, np.int32)
    for l in range(levels):
        visible = occs[l] >= 0
        if warmup:
            got = np.nonzero(visible)[0]
        else:
            draws = np.asarray(cell_draws[l], np.int64)
            uniform = draws[visible[draws]]                      # draws on invisible cells are dropped, order kept
            occupied = np.nonzero(binaries[l] & visible)[0]      # ascending cell order
            if len(occupied) > n:
                u = np.asarray(sel_draws[l], f32)
                k = np.minimum((u * f32(len(occupied))).astype(np.int64), len(occupied) - 1)  # fp32 product, truncated
                occupied = occupied[k]
            got = np.concatenate([uniform, occupied])
        ids[l, :len(got)] = got
        counts[l] = len(got)
    return ids, counts


def cell_xyz(ids, res):
    ids = np.asarray(ids, np.int64)
    return np.stack([ids // (res * res), (ids // res) % res, ids % res], -1)


def positions(aabbs, res, ids, jitter, dtype=f32):
    """[L,cap,3]: x = (cell_xyz + jitter) / res, p = lo + x (hi - lo), every step rounded to ``dtype``; padded slots (-1) sit at
    the centre of their level's box.  dtype=float64 evaluates the same formula on the same fp32 inputs without rounding."""
    aabbs = np.asarray(aabbs, f32)
    L = ids.shape[0]
    lo, hi = aabbs[:, None, :3].astype(dtype), aabbs[:, None, 3:].astype(dtype)
    x = (cell_xyz(np.maximum(ids, 0), res).astype(dtype) + np.asarray(jitter, f32).astype(dtype)) / dtype(res)
    p = lo + x * (hi - lo)
    centre = ((lo + hi) * dtype(0.5)).astype(dtype)
    return np.where((ids >= 0)[..., None], p, np.broadcast_to(centre, p.shape)).astype(dtype).reshape(L, -1, 3)


def cell_faces_f32(aabbs, res, ids):
    """the cells' faces (lo, hi) [L,cap,3] in the update's own fp32 arithmetic: lo + (k / res) (hi - lo) at k = c and c + 1.
    Every step of the position formula is monotone in the jitter, so a position lies between these EXACTLY, for any box."""
    aabbs = np.asarray(aabbs, f32)
    lo, ext = aabbs[:, None, :3], aabbs[:, None, 3:] - aabbs[:, None, :3]
    c = cell_xyz(np.maximum(ids, 0), res).astype(f32)
    return lo + (c / f32(res)) * ext, lo + ((c + f32(1)) / f32(res)) * ext


def cell_boxes(aabbs, res, ids):
    """closed float64 boxes (lo, hi) [L,cap,3] of the candidates' cells"""
    aabbs = np.asarray(aabbs, f32).astype(f64)
    lo, ext = aabbs[:, None, :3], aabbs[:, None, 3:] - aabbs[:, None, :3]
    c = cell_xyz(np.maximum(ids, 0), res).astype(f64)
    return lo + c / res * ext, lo + (c + 1.0) / res * ext


# ---- EMA and threshold -----------------------------------------------------------------------------------------------------
def ema(occs, res, ids, counts, values, decay):
    """occs[c] = max(occs[c] * decay, max of the cell's candidate values), decay once per touched cell (fp32).  A NaN value is
    ignored as if its candidate were absent; a NaN in occs fails occs >= 0 and is treated as invisible."""
    L, cap = ids.shape
    cells = res ** 3
    out = np.asarray(occs, f32).reshape(L, cells).copy()
    values = np.asarray(values, f32).reshape(L, cap)
    for l in range(L):
        c, v = ids[l, :counts[l]].astype(np.int64), values[l, :counts[l]]
        ok = (c >= 0) & (c < cells) & ~np.isnan(v)  # a NaN value counts as no candidate
        c, v = c[ok], v[ok]
        m = np.full(cells, -np.inf, f32)
        np.maximum.at(m, c, v)
        touched = np.zeros(cells, bool)
        touched[c] = True
        touched &= out[l] >= 0  # invisible cells are never written
        out[l][touched] = np.maximum(out[l][touched] * f32(decay), m[touched])
    return out.reshape(-1)


def threshold(occs, occ_thre):
    """-> (binaries bool [N], thre fp32, mean float64): mean of the visible occs in float64, rounded to fp32 once"""
    occs = np.asarray(occs, f32).reshape(-1)
    vis = occs >= 0
    if not vis.any():
        return np.zeros(occs.shape, bool), f32(np.inf), np.nan
    mean = occs[vis].astype(f64).sum() / vis.sum()
    thre = min(f32(mean), f32(occ_thre))
    return occs > thre, f32(thre), mean


def threshold_gap(occs, thre):
    """smallest relative distance |occ - thre| / thre of a visible cell's value to the threshold"""
    occs = np.asarray(occs, f64).reshape(-1)
    return float(np.min(np.abs(occs[occs >= 0] - f64(thre))) / f64(thre))


def update(aabbs, res, occs, binaries, occ_fn, step, warmup_steps, occ_thre, decay, jitter, cell_draws=None, sel_draws=None,
           n=None):
    """one whole update -> dict(ids, counts, positions, occs, binaries, thre, mean)"""
    L = np.asarray(aabbs).shape[0]
    ids, counts = candidates(occs, binaries, res, L, step < warmup_steps, n, cell_draws, sel_draws)
    pos = positions(aabbs, res, ids, jitter)
    vals = np.asarray(occ_fn(pos.reshape(-1, 3)), f32).reshape(L, -1)
    new = ema(occs, res, ids, counts, vals, decay)
    b, thre, mean = threshold(new, occ_thre)
    return dict(ids=ids, counts=counts, positions=pos, occs=new, binaries=b.reshape(L, res, res, res), thre=thre, mean=mean)


# ---- invisible cells -------------------------------------------------------------------------------------------------------
def mark_invisible(aabbs, res, K, c2w, width, height, near_plane, dtype=f32, margin=None):
    """-> visible bool [L*res^3] (and, with ``margin``, ambiguous bool: some camera's u, v or depth test lies within
    ``margin`` of its bound).  Cell point lo + idx/(res-1) (hi-lo); cam = R^T (x - t), h = K cam, z = h[2], u = h[0]/z,
    v = h[1]/z, sums left to right in ``dtype``."""
    aabbs = np.asarray(aabbs, f32).astype(dtype)
    K = np.broadcast_to(np.asarray(K, f32), (len(c2w), 3, 3)).astype(dtype)
    M = np.asarray(c2w, f32)[:, :3, :4].astype(dtype)
    L = aabbs.shape[0]
    idx = cell_xyz(np.arange(res ** 3), res).astype(dtype)
    frac = idx / dtype(max(res - 1, 1))
    vis, amb = [], []
    for l in range(L):
        x = aabbs[l, :3] + frac * (aabbs[l, 3:] - aabbs[l, :3])
        seen = np.zeros(len(x), bool)
        too_near = np.zeros(len(x), bool)
        unsure = np.zeros(len(x), bool)
        for n in range(len(M)):
            d = x - M[n, :, 3]
            cam = [(M[n, 0, i] * d[:, 0] + M[n, 1, i] * d[:, 1]) + M[n, 2, i] * d[:, 2] for i in range(3)]
            h = [(K[n, i, 0] * cam[0] + K[n, i, 1] * cam[1]) + K[n, i, 2] * cam[2] for i in range(3)]
            with np.errstate(divide="ignore", invalid="ignore"):
                z, u, v = h[2], h[0] / h[2], h[1] / h[2]
                in_image = (z >= 0) & (u >= 0) & (u < dtype(width)) & (v >= 0) & (v < dtype(height))
                seen |= in_image & (z >= dtype(near_plane))
                too_near |= in_image & (z < dtype(near_plane))
                if margin is not None:
                    for val, bound in ((z, 0.0), (z, near_plane), (u, 0.0), (u, width), (v, 0.0), (v, height)):
                        unsure |= ~(np.abs(val - bound) >= margin)  # NaN counts as unsure
        vis.append(seen & ~too_near)
        amb.append(unsure)
    vis = np.concatenate(vis)
    return vis if margin is None else (vis, np.concatenate(amb))


# ---- multi-level march -----------------------------------------------------------------------------------------------------
def march_levels(aabbs, binaries, origins, dirs, step, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None,
                 cone_angle=0.0, max_candidates=1 << 16, margin=1e-4):
    """Every candidate interval of every ray, in order: dict of arrays ray, t_start, t_end (fp32), keep, ambiguous.
    The ray is clipped to the outermost box; a candidate's level is the first whose closed box contains its midpoint
    (the outermost when none does); kept iff that level's cell -- floor((p - lo)/(hi - lo) * res), clamped -- is set.
    ``ambiguous``: the float64 midpoint lies within ``margin`` of a cell face of its level, in units of that cell, or within
    ``margin`` of a level's box face, in units of the cell of the level whose box it is."""
    aabbs = np.asarray(aabbs, f32)
    binaries = np.asarray(binaries).astype(bool)
    L, res = binaries.shape[0], binaries.shape[-1]
    lo, hi = aabbs[:, :3], aabbs[:, 3:]
    out = dict(ray=[], t_start=[], t_end=[], keep=[], ambiguous=[])
    for r in range(origins.shape[0]):
        o, d = origins[r].astype(f32), dirs[r].astype(f32)
        near = max(f32(near_plane), f32(t_min[r]) if t_min is not None else f32(near_plane))
        far = min(f32(far_plane), f32(t_max[r]) if t_max is not None else f32(far_plane))
        tn, tf, ok = f32(near), f32(far), True
        for a in range(3):
            if d[a] == 0:
                ok &= bool(lo[-1][a] <= o[a] <= hi[-1][a])
                continue
            inv = f32(1) / d[a]
            ta, tb = (lo[-1][a] - o[a]) * inv, (hi[-1][a] - o[a]) * inv
            if ta > tb:
                ta, tb = tb, ta
            tn, tf = max(tn, ta), min(tf, tb)
        if not ok or not (tn < tf):
            continue
        k1, t1 = 0, tn
        if cone_angle > 0 and tn * f32(cone_angle) < f32(step):
            k1 = int(np.ceil((f32(step) / f32(cone_angle) - tn) / f32(step)))
            t1 = f32(tn + f32(k1) * f32(step))

        def at(k):
            if cone_angle <= 0 or k < k1:
                return f32(tn + f32(k) * f32(step))
            return f32(t1 * f32(np.power(f64(f32(1) + f32(cone_angle)), f64(k - k1))))

        for k in range(max_candidates):
            ts = at(k)
            if not ts < tf:
                break
            te = min(at(k + 1), tf)
            if not te > ts:
                continue
            tm = f32(0.5) * (ts + te)
            p = o + d * tm
            lvl = L - 1
            for l in range(L - 1):
                if np.all(p >= lo[l]) and np.all(p <= hi[l]):
                    lvl = l
                    break
            u = (p - lo[lvl]) / (hi[lvl] - lo[lvl])
            idx = np.clip(np.floor(u * f32(res)).astype(np.int64), 0, res - 1)
            # float64 view of the same midpoint: distance to the nearest cell face of its level and to every level's box
            p64 = o.astype(f64) + d.astype(f64) * (0.5 * (f64(ts) + f64(te)))
            cell = (hi[lvl].astype(f64) - lo[lvl]) / res
            g = (p64 - lo[lvl]) / cell
            amb = bool(np.any(np.abs(g - np.round(g)) < margin))
            for l in range(L):
                cl = (hi[l].astype(f64) - lo[l]) / res
                amb |= bool(np.any(np.abs(p64 - lo[l]) / cl < margin) or np.any(np.abs(p64 - hi[l]) / cl < margin))
            out["ray"].append(r), out["t_start"].append(ts), out["t_end"].append(te)
            out["keep"].append(bool(binaries[lvl, idx[0], idx[1], idx[2]])), out["ambiguous"].append(amb)
    return dict(ray=np.asarray(out["ray"], np.int64), t_start=np.asarray(out["t_start"], f32),
                t_end=np.asarray(out["t_end"], f32), keep=np.asarray(out["keep"], bool),
                ambiguous=np.asarray(out["ambiguous"], bool))


# ---- scenarios shared by the CPU and the GPU tests ------------------------------------------------------------------------
SHELL_STEPS = [0, 16, 256, 272]  # two warm-up updates, two after it (warmup_steps = 256)


def shell_run(occ_thre, res=32, levels=2):
    """the threshold scenario of the GPU test, in numpy: yields (step, draws, result) of every update"""
    aabbs = level_aabbs([-1, -1, -1, 1, 1, 1], levels)
    occs, binaries = np.zeros(levels * res ** 3, np.float32), np.ones((levels, res, res, res), bool)
    for i, step in enumerate(SHELL_STEPS):
        d = draws(res, levels, step < 256, 100 + i)
        out = update(aabbs, res, occs, binaries, shell_occ, step, 256, occ_thre, 0.95, d["jitter"], d["cell_draws"],
                        d["sel_draws"])
        occs, binaries = out["occs"], out["binaries"]
        yield step, d, out


def cameras(n=10, seed=0):
    """OpenCV cameras around and inside [-4,4]^3, looking roughly at the origin -> K [n,3,3], c2w [n,3,4], width, height"""
    rng = np.random.default_rng(seed)
    c2w = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        t = rng.uniform(-3.0, 3.0, 3) if i < n // 2 else rng.uniform(5.0, 7.0, 3) * rng.choice([-1.0, 1.0], 3)
        z = -t / np.linalg.norm(t) + rng.normal(0, 0.2, 3)
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        c2w[i, :, 0], c2w[i, :, 1], c2w[i, :, 2], c2w[i, :, 3] = x, np.cross(z, x), z, t
    K = np.tile(np.array([[90.0, 0.0, 32.0], [0.0, 90.0, 24.0], [0.0, 0.0, 1.0]], np.float32), (n, 1, 1))
    K[:, 0, 0] += rng.uniform(-5, 5, n).astype(np.float32)
    return K, c2w, 64, 48
