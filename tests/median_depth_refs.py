"""The median-depth contract (include/neurad_hip.h at nrhip_median_depth) restated in numpy, and the inputs the fixture
tests/golden/median_depth.npz and the GPU tests share.

    c_i = float32(float64 running sum of the fp32 weights, in sample order)      (np.cumsum in float64, cast once)
    k   = the first i with not (c_i < q), else n - 1                             (a NaN c_i crosses where it stands)
    depth = NaN if c_k is NaN else (start_k + end_k) * 0.5 in fp32,  index = k;  a ray without samples: 0 and -1

Pinned bit for bit to the reference's own DepthRenderer("median") on the CPU by tests/test_median_depth_refs_host.py."""
import math

import numpy as np

import synth

F32 = np.float32
UNIT = 2.0 ** -24  # every fixture weight is a multiple of it below 2: float64 partial sums are exact in any order
SHAPES = (1, 2, 63, 64, 65, 129, 200)  # S on either side of the 64-sample chunk and its carry
R = 300  # not a multiple of any rays-per-block
PACKED_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 200)


def median_depth_ray(w, starts, ends, q=0.5):
    """one ray -> (depth fp32, index)"""
    w = np.asarray(w, F32)
    n = w.shape[0]
    if n == 0:
        return F32(0.0), -1
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.cumsum(w.astype(np.float64)).astype(F32)
    crossed = ~(c < F32(q))
    k = int(np.argmax(crossed)) if crossed.any() else n - 1
    if np.isnan(c[k]):
        return F32(np.nan), k
    with np.errstate(invalid="ignore", over="ignore"):
        return F32(F32(F32(starts[k]) + F32(ends[k])) * F32(0.5)), k


def median_depth(w, starts, ends, thresholds=(0.5,)):
    """dense [R,S] -> depth fp32 [R,K], index int32 [R,K]"""
    Rn, K = w.shape[0], len(thresholds)
    depth, index = np.zeros((Rn, K), F32), np.zeros((Rn, K), np.int32)
    for r in range(Rn):
        for j, q in enumerate(thresholds):
            depth[r, j], index[r, j] = median_depth_ray(w[r], starts[r], ends[r], q)
    return depth, index


def median_depth_packed(w, starts, ends, segments, thresholds=(0.5,)):
    """packed [M] with segments [R+1] -> depth fp32 [R,K], index int32 [R,K]"""
    Rn, K = len(segments) - 1, len(thresholds)
    depth, index = np.zeros((Rn, K), F32), np.zeros((Rn, K), np.int32)
    for r in range(Rn):
        a, b = int(segments[r]), int(segments[r + 1])
        for j, q in enumerate(thresholds):
            depth[r, j], index[r, j] = median_depth_ray(w[a:b], starts[a:b], ends[a:b], q)
    return depth, index


def partial_sums_exact(w, unit_log2=-24) -> bool:
    """are the float64 partial sums of every row exact (so that every order of the additions gives the same ones)?  The
    sums are recomputed in integers, in units of 2^unit_log2, of which every weight has to be a multiple; the sequential
    float64 sum and math.fsum have to equal them at every sample.  A +inf ends a row: behind it every sum is +inf."""
    unit = 2.0 ** unit_log2
    for row in np.atleast_2d(w):
        total, acc, seen = 0, 0.0, []
        for v in (float(x) for x in row):
            if v == math.inf:
                break
            u = int(round(v / unit))
            if not math.isfinite(v) or u * unit != v:
                return False
            total += u
            acc += v
            seen.append(v)
            if abs(total) >= 2 ** 53 or acc != total * unit or math.fsum(seen) != acc:
                return False
    return True


# ---- inputs -------------------------------------------------------------------------------------------------------------
def checksum(a):
    """[R,S] -> float64 [R]: the rows' sequential float64 sums, what the fixture keeps of the regenerated inputs"""
    return np.add.accumulate(a.astype(np.float64), axis=-1)[:, -1]



def weights(n_rays, n, seed):
    """rand**8 (a few samples carry the ray), normalised per ray to a total drawn from [0, 1.5), rounded to multiples of
    2^-24: about a third of the rays never reach one half"""
    if n == 0:
        return np.zeros((n_rays, 0), F32)
    u = synth.uniform((n_rays, n), 0.0, 1.0, seed).astype(np.float64)
    for _ in range(3):  # u ** 8 by squaring, and the row total as a sequential sum: plain IEEE operations in a fixed order,
        u = u * u       # so every machine regenerates the same weights (the fixture pins their sums)
    total = synth.uniform((n_rays, 1), 0.0, 1.5, seed + 1).astype(np.float64)
    w = u / np.maximum(np.add.accumulate(u, axis=-1)[:, -1:], 1e-300) * total
    return (np.round(w / UNIT) * UNIT).astype(F32)


def edges(n_rays, n, seed):
    """sorted uniform draws in [0, 100) -> starts, ends [n_rays, n]"""
    e = np.sort(synth.uniform((n_rays, n + 1), 0.0, 100.0, seed), axis=-1)
    return np.ascontiguousarray(e[:, :-1]), np.ascontiguousarray(e[:, 1:])


def place_crossings(w):
    """rows 0-4 of a dense batch get their crossing of one half at sample 0, 63, 64, S - 1 and never (where S has them)"""
    S = w.shape[1]
    for row, at in enumerate((0, 63, 64, S - 1, None)):
        if row >= w.shape[0] or (at is not None and at >= S):
            continue
        w[row] = F32(UNIT * 3)
        if at is None:
            w[row] = F32(0.25 / S if S > 1 else 0.25)
            w[row] = (np.round(w[row].astype(np.float64) / UNIT) * UNIT).astype(F32)
        else:
            w[row, at] = F32(0.75)
    return w


def dense_case(S, seed=None):
    """the fixture's dense batch of R rays with S samples -> weights, starts, ends"""
    seed = 1000 + 10 * S if seed is None else seed
    s, e = edges(R, S, seed + 2)
    return place_crossings(weights(R, S, seed)), s, e


def constructed_rays():
    """name -> (weights [12], expected index): the rays that tell an fp32 accumulator, a float64 comparison, an ignored +inf
    and a missing clamp from the contract"""
    n = 12
    tiny = np.full(n, 2.0 ** -28, F32)
    tiny[0] = F32(0.5 - 2.0 ** -25)  # fp32 accumulation never moves off 0.5 - 2^-25; float64: 0.5 - 2^-26 rounds up at i = 4
    tie = np.zeros(n, F32)
    tie[:3] = (0.25, 0.25 - 2.0 ** -27, 0.25)  # (0.25 - 2^-27 is half an fp32 ulp below 0.25 and is stored as 0.25)
    half = np.zeros(n, F32)
    half[:3] = (0.25, 0.25 - 2.0 ** -26, 0.25)  # the float64 sum 0.5 - 2^-26 is below one half, float32 of it IS one half
    inf = np.zeros(n, F32)
    inf[3] = np.inf
    return {"fp32_accumulator": (tiny, 4), "tie": (tie, 1), "float64_compare": (half, 1), "inf": (inf, 3),
            "never": (np.full(n, 0.04, F32), n - 1)}


def constructed_case():
    """-> weights [5,12], starts, ends, expected index [5]"""
    rays = constructed_rays()
    w = np.stack([v[0] for v in rays.values()])
    s, e = edges(len(rays), w.shape[1], 77)
    return w, s, e, np.array([v[1] for v in rays.values()], np.int32)


def packed_case(n_rays=R, seed=500):
    """segment lengths PACKED_LENGTHS in a shuffled order, an empty ray first and last -> weights, starts, ends [M],
    segments int64 [R+1], counts"""
    pick = (synth.uniform((n_rays,), 0.0, len(PACKED_LENGTHS), seed) % len(PACKED_LENGTHS)).astype(np.int64)
    counts = np.array(PACKED_LENGTHS, np.int64)[pick]
    counts[: len(PACKED_LENGTHS)] = PACKED_LENGTHS[::-1]  # every length occurs
    counts[0] = counts[-1] = 0
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    w, s, e = [], [], []
    for r, n in enumerate(counts):
        w.append(weights(1, int(n), seed + 3 * r + 1)[0])
        a, b = edges(1, int(n), seed + 3 * r + 2)
        s.append(a[0]), e.append(b[0])
    return np.concatenate(w).astype(F32), np.concatenate(s).astype(F32), np.concatenate(e).astype(F32), seg, counts
