"""The binned table gradient's float64 reference and its per-entry fixed-point bound (csrc/encode_bwd_binned.hip), shared by
the tests of every source that goes through the partition (tests/test_gpu_table_grad_precision.py has the derivation)."""
import numpy as np

import neurad_oracle as O

U = 2.0 ** -24


def log2_slice(L, F, lg, n_slots=1):
    """entries per slice (log2) as make_plan sets it"""
    ts = min(14 - (F - 1).bit_length(), lg)
    while ((L * n_slots) << (lg - ts)) < 512 and ts > 9:
        ts -= 1
    return ts


def quantum(vmax, records, pair):
    """the kernel's q = 2^-sh for a slice: vmax = the level's max |record value|, records = the slice's record count"""
    e = np.frexp(vmax)[1] - 1  # 2^e <= vmax < 2^(e+1)
    hb = np.array([int(r).bit_length() for r in np.ravel(records)]).reshape(np.shape(records)) + (1 if pair else 0)
    return np.ldexp(1.0, -(61 - hb - (e + 1)))


def reference(x, go, L, F, lg, mn, mx, n_slots=1):
    """float64 index_add of the exact corner terms -> per entry (g, a, n) and per (level, slice) (max |term|, max a,
    terms) -- the last three bound the kernel's vmax and record counts"""
    scal = O.hash_scalings(L, mn, mx)
    T = 1 << lg
    idx, off = O.hashgrid_corner_indices(x, scal, T)  # [N, L, 8] (with the level offset), [N, L, 3]
    o = off.astype(np.float64)
    ox, oy, oz = o[..., 0], o[..., 1], o[..., 2]
    cx, fx, cy, fy, cz, fz = ox, 1 - ox, oy, 1 - oy, oz, 1 - oz
    # corner order of hashgrid_corner_indices: (c,c,c) (c,f,c) (f,f,c) (f,c,c) (c,c,f) (c,f,f) (f,f,f) (f,c,f)
    w = np.stack([cx * cy * cz, cx * fy * cz, fx * fy * cz, fx * cy * cz, cx * cy * fz, cx * fy * fz, fx * fy * fz,
                  fx * cy * fz], -1)
    g = go.reshape(-1, L, F).astype(np.float64)
    terms = w[..., None] * g[:, :, None, :]  # [N, L, 8, F]
    live = (go != 0).any(-1)  # rows of +-0 send no records
    key = (idx[..., None] * F + np.arange(F)).reshape(-1)
    size = L * T * F
    ref = np.bincount(key, terms.reshape(-1), size)
    a = np.bincount(key, np.abs(terms).reshape(-1), size)
    n = np.bincount(key, np.broadcast_to(live[:, None, None, None], terms.shape).reshape(-1).astype(np.float64), size)
    ts = log2_slice(L, F, lg, n_slots)
    ent = idx - (np.arange(L) * T)[None, :, None]
    sl = (np.arange(L)[None, :, None] << (lg - ts)) + (ent >> ts)
    nsl = L << (lg - ts)
    recs = np.bincount(sl[live].reshape(-1), minlength=nsl).astype(np.float64) * F
    tmax = np.abs(terms).reshape(len(x), L, -1).max((0, 2)) if len(x) else np.zeros(L)
    amax = a.reshape(L, -1).max(1)
    return ref, a, n, recs, tmax, amax, ts


def bound_for(ref, a, n, recs, tmax, amax, ts, L, F, lg, pair):
    vmax = np.minimum(16 * tmax, amax) * (1 + 64 * U)  # a record merges at most 16 terms of one entry
    ns = 1 << (lg - ts)
    q_slice = quantum(np.repeat(vmax, ns), recs, pair)  # [L * slices]
    q = np.repeat(q_slice, (1 << ts) * F)  # per entry
    return n * q / 2 + 32 * U * a + U * np.abs(ref), q


def check_entries(got, ref, bnd, what):
    err = np.abs(got - ref)
    over = ~(err <= bnd)
    if over.any():
        k = int(np.argmax(over))
        raise AssertionError(f"{what}: {int(over.sum())} entries off the fixed-point bound, first {k}: got {got[k]!r} want "
                             f"{ref[k]!r} bound {bnd[k]!r}")
