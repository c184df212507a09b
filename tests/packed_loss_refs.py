"""What the tests of the packed loss kernels share (csrc/losses.hip: nrhip_packed_distortion_loss,
nrhip_packed_lidar_carving): the ragged test rays, generated from seeds, and numpy restatements of the two contracts of
include/neurad_hip.h -- the prefix form of the distortion loss written sequentially in float64, an independent O(n^2)
float64 form on exactly rounded sums (math.fsum), the carving mask and loss in the kernels' own precision -- with the error
bounds of the header as functions.  No kernel code is shared.  tests/golden/packed_losses.npz holds the reference's own
results for these inputs (scripts/make_golden_packed_losses.py)."""
import functools
import math
import os

import numpy as np

from packed_restatement import segments_from_counts
from packed_train_refs import RAGGED

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_losses.npz")
COUNTS = RAGGED + (1000,)  # every chunking of a wave of 64: 0, 1, around 16 / 32 / 64 / 128, a carried scan, a long ray
GOLD_COUNTS = RAGGED       # the rays the reference's O(n^2) expression is recorded for
C_BOUND = 16               # NRHIP_PACKED_DISTORTION_C: derived in include/neurad_hip.h
U64, U32 = 2.0 ** -53, 2.0 ** -24
KINDS = ("gapped", "contiguous", "tied", "zero_width")
EPS, NON_RETURN = 0.5, 150.0  # carving_epsilon, non_return_lidar_distance of the carving case


def kind_of(ray):
    return KINDS[ray % 4]


def _intervals(rng, n, kind):
    """n sorted intervals in [0, 1) with non-decreasing midpoints"""
    if kind == "contiguous":
        edges = np.sort(rng.uniform(0.0, 1.0, n + 1))
        return edges[:-1], edges[1:]
    edges = np.sort(rng.uniform(0.0, 1.0, 2 * n))
    s, e = edges[0::2].copy(), edges[1::2].copy()
    if kind == "tied":  # every third interval repeats the one before it: equal midpoints
        for k in range(1, n, 3):
            s[k], e[k] = s[k - 1], e[k - 1]
    if kind == "zero_width":  # every third interval has no width
        e[::3] = s[::3]
    return s, e


@functools.lru_cache(maxsize=None)
def distortion_case(counts=COUNTS, seed=20):
    """-> s, e, w fp32 [M], seg int64 [R+1].  Ray r is of kind_of(r); odd rays are in metres (x 60), even ones in [0, 1);
    the weights are peaked (a narrow bump on a small floor, what the loss produces), with exact zeros among them."""
    rng = np.random.default_rng(seed)
    S, E, W = [], [], []
    for r, n in enumerate(counts):
        s, e = _intervals(rng, n, kind_of(r))
        scale = 60.0 if r % 2 else 1.0
        i = np.arange(n)
        w = np.exp(-0.5 * ((i - rng.uniform(0, max(n, 1))) / max(0.03 * n, 0.7)) ** 2) + 1e-3 * rng.uniform(0, 1, n)
        w = 0.9 * w / max(w.sum(), 1e-30) * rng.uniform(0.2, 1.0)
        w[rng.uniform(0, 1, n) < 0.1] = 0.0
        S.append(s * scale), E.append(e * scale), W.append(w)
    cat = lambda parts: np.concatenate(parts).astype(np.float32)  # noqa: E731
    s, e = cat(S), cat(E)
    e = np.maximum(s, e)  # (rounding to fp32 is monotone: order and widths >= 0 are kept)
    return s, e, cat(W), segments_from_counts(counts)


# ---- the distortion loss ------------------------------------------------------------------------------------------------
def distortion_prefix(s, e, w, seg):
    """the contract of nrhip_packed_distortion_loss written sequentially in float64 (before the one rounding to fp32)
    -> loss [R], grad [M]"""
    s, e, w = (np.asarray(a, np.float64) for a in (s, e, w))
    loss, grad = np.zeros(len(seg) - 1), np.zeros(len(w))
    for r in range(len(seg) - 1):
        b, n = int(seg[r]), int(seg[r + 1] - seg[r])
        m, d, wr = (s[b:b + n] + e[b:b + n]) / 2, e[b:b + n] - s[b:b + n], w[b:b + n]
        A, B = np.zeros(n + 1), np.zeros(n + 1)
        for i in range(n):
            A[i + 1], B[i + 1] = A[i] + wr[i], B[i] + wr[i] * m[i]
        W, Bt = A[n], B[n]
        inter = intra = 0.0
        for i in range(n):
            inter += wr[i] * (m[i] * A[i] - B[i])
            intra += wr[i] * wr[i] * d[i]
            grad[b + i] = 2.0 * (m[i] * (A[i] - (W - A[i] - wr[i])) - (B[i] - (Bt - B[i] - wr[i] * m[i]))) \
                + (2.0 / 3.0) * wr[i] * d[i]
        loss[r] = 2.0 * inter + intra / 3.0
    return loss, grad


def distortion_quadratic(s, e, w, seg):
    """the reference's expression sum_ij w_i w_j |m_i - m_j| + sum_i w_i^2 delta_i / 3 and its derivative w.r.t. w in
    float64, every sum exactly rounded (math.fsum) -> loss [R], grad [M]"""
    s, e, w = (np.asarray(a, np.float64) for a in (s, e, w))
    loss, grad = np.zeros(len(seg) - 1), np.zeros(len(w))
    for r in range(len(seg) - 1):
        b, n = int(seg[r]), int(seg[r + 1] - seg[r])
        m, d, wr = (s[b:b + n] + e[b:b + n]) / 2, e[b:b + n] - s[b:b + n], w[b:b + n]
        dist = np.abs(m[:, None] - m[None, :])
        rows = [math.fsum(wr * dist[i]) for i in range(n)]  # sum_j w_j |m_i - m_j|
        loss[r] = math.fsum((wr[:, None] * wr[None, :] * dist).ravel()) + math.fsum(wr * wr * d) / 3.0
        grad[b:b + n] = [2.0 * rows[i] + (2.0 / 3.0) * wr[i] * d[i] for i in range(n)]
    return loss, grad


def distortion_scales(s, e, w, seg):
    """per ray: n, X = max |m|, S = sum |w| (float64) -- what the error bounds of the header are stated in"""
    s, e, w = (np.asarray(a, np.float64) for a in (s, e, w))
    R = len(seg) - 1
    n = np.diff(np.asarray(seg, np.int64)).astype(np.float64)
    X, S = np.zeros(R), np.zeros(R)
    for r in range(R):
        b, c = int(seg[r]), int(seg[r + 1])
        if c > b:
            X[r], S[r] = np.abs((s[b:c] + e[b:c]) / 2).max(), np.abs(w[b:c]).sum()
    return n, X, S


def float64_term(n, X, S, power):
    """c (n + 2) 2^-53 X S^power: the float64 prefix sums' rounding through the cancellation (power 2: loss, 1: gradient)"""
    return C_BOUND * (n + 2) * U64 * X * S ** power


def loss_bound(ref, n, X, S):
    """|loss - ref| <= 2^-24 |ref| + c (n + 2) 2^-53 X S^2, per ray"""
    return U32 * np.abs(ref) + float64_term(n, X, S, 2)


def grad_bound(ref, n, X, S, seg):
    """|grad_k - ref_k| <= 2^-24 |ref_k| + c (n + 2) 2^-53 X S, per sample (n, X, S of the sample's ray)"""
    rep = np.diff(np.asarray(seg, np.int64))
    return U32 * np.abs(ref) + np.repeat(float64_term(n, X, S, 1), rep)


# ---- lidar carving ------------------------------------------------------------------------------------------------------
def _around(rng, n, lo, hi):
    """n sorted contiguous intervals over [lo, hi]"""
    edges = np.sort(rng.uniform(lo, hi, n + 1)).astype(np.float32)
    return edges[:-1].copy(), edges[1:].copy()


def _place(ts, te, k, mid, half=0.25):
    """sample k: an interval whose fp32 midpoint (start + end) * 0.5 is exactly `mid`"""
    mid = np.float32(mid)
    ts[k], te[k] = mid - np.float32(half), mid + np.float32(half)
    assert (ts[k] + te[k]) * np.float32(0.5) == mid, (k, mid)


@functools.lru_cache(maxsize=None)
def carving_case(counts=COUNTS, seed=21):
    """-> dict: t_starts, t_ends, weights fp32 [M], seg, is_lidar / did_return bool [R], distance fp32 [R].  Rays cycle
    through camera, returned lidar, non-returned lidar; a returned ray's samples crowd around its measured distance, a
    non-returned one's around non_return_lidar_distance.  Rays 13 and 14 (65 and 130 samples) carry the boundary samples:
    ray 13 returned at distance 10 with midpoints exactly on 10 -+ eps and one float inside either, ray 14 not returned
    with midpoints exactly on non_return_lidar_distance and one float below it."""
    rng = np.random.default_rng(seed)
    R = len(counts)
    is_lidar = np.array([r % 3 != 0 for r in range(R)])
    did_return = np.array([r % 3 == 1 for r in range(R)])
    distance = rng.uniform(5.0, 60.0, R).astype(np.float32)
    is_lidar[13], did_return[13], distance[13] = True, True, 10.0
    is_lidar[14], did_return[14] = True, False
    is_lidar[R - 1], did_return[R - 1] = True, True  # the long ray: returned lidar
    TS, TE = [], []
    for r, n in enumerate(counts):
        if is_lidar[r] and did_return[r]:
            ts, te = _around(rng, n, max(distance[r] - 3 * EPS, 0.05), distance[r] + 3 * EPS)
        elif is_lidar[r]:
            ts, te = _around(rng, n, NON_RETURN - 40.0, NON_RETURN + 40.0)
        else:
            ts, te = _around(rng, n, 0.1, 60.0)
        TS.append(ts), TE.append(te)
    f = np.float32
    lo, hi = f(10.0 - EPS), f(10.0 + EPS)
    for k, mid in enumerate((lo, np.nextafter(lo, f(np.inf)), np.nextafter(hi, f(-np.inf)), hi)):
        _place(TS[13], TE[13], 20 + k, mid)  # not close, close, close, not close
    for k, mid in enumerate((np.nextafter(f(NON_RETURN), f(-np.inf)), f(NON_RETURN))):
        _place(TS[14], TE[14], 30 + k, mid, half=1.0)  # close, not close
    seg = segments_from_counts(counts)
    M = int(seg[-1])
    w = (rng.uniform(0.0, 1.0, M) ** 4).astype(np.float32)
    w[rng.uniform(0, 1, M) < 0.1] = 0.0
    cat = lambda parts: np.concatenate(parts).astype(np.float32)  # noqa: E731
    return {"t_starts": cat(TS), "t_ends": cat(TE), "weights": w, "seg": seg, "is_lidar": is_lidar,
            "did_return": did_return, "distance": distance}


def carving_mask(ts, te, seg, is_lidar, did_return, distance, eps=EPS, non_return=NON_RETURN):
    """the mask as the header states it, in fp32: mid = (t_start + t_end) * 0.5f, both comparisons strict -> bool [M]"""
    rep = np.diff(np.asarray(seg, np.int64))
    lid = np.repeat(np.asarray(is_lidar, bool), rep)
    ret = np.ones_like(lid) if did_return is None else np.repeat(np.asarray(did_return, bool), rep)
    dist = np.repeat(np.asarray(distance, np.float32), rep)
    mid = (np.asarray(ts, np.float32) + np.asarray(te, np.float32)) * np.float32(0.5)
    near = np.abs(dist - mid) < np.float32(eps)
    return lid & np.where(ret, near, mid < np.float32(non_return))


def carving_loss(w, close, seg, is_lidar):
    """-> loss [R] float64 (= sum wf^2: exactly rounded sums of the exact squares), grad fp32 [M] = 2 wf"""
    rep = np.diff(np.asarray(seg, np.int64))
    far = np.repeat(np.asarray(is_lidar, bool), rep) & ~np.asarray(close, bool)
    wf = np.where(far, np.asarray(w, np.float32), np.float32(0.0)).astype(np.float32)
    sq = wf.astype(np.float64) ** 2
    loss = np.array([math.fsum(sq[int(seg[r]):int(seg[r + 1])]) for r in range(len(seg) - 1)])
    return loss, np.float32(2.0) * wf


def carving_loss_bound(ref, n, sum_sq):
    """|loss - ref| <= 2^-24 |ref| + n 2^-53 sum wf^2, per ray"""
    return U32 * np.abs(ref) + n * U64 * sum_sq


def gold():
    return np.load(GOLDEN)
