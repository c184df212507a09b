"""Ray gradients through the pair positions of PACKED samples (nrhip_actor_pair_positions_bwd_rays_packed): what
tests/test_gpu_packed_actor_ray_grads.py and tests/test_packed_actor_ray_grads_host.py share.  No GPU, no test functions.

GENERIC tier: a dense [R,S] scene of tests/actor_refs.py handed to the packed kernel -- as uniform segments, or cut to a
per-ray prefix of its samples (`cut`: CUT's lengths in turn, 0 samples included) with the pair indices remapped.  A pair's
contribution depends on its ray and its interval only, so the float64 reference of either layout is actor_refs.pair_case on
the DENSE scene with the pairs that survive the cut, and the bound is actor_refs.pair_grad_bound(ref, key, dpp=log2 G): a
lane's chain is at most n_ray additions and the butterfly adds log2 G roundings, both on the sum S of the contributions'
magnitudes -- the (n + dpp) S term of that bound.

EXACT tier (`exact_case`): every contribution is a dyadic number, so the sums are exact in any order and the kernel must
equal the float64 value bit for bit.  Parked actors with stored rotations (1,0,0, 0,1,0) (both Gram-Schmidt steps and the
lerp are exact; the box frame is the world frame moved by the actor's position), actor_scale 32 with every box position
below 32 in every axis (the uncontracted branch: d x01 / d pos = 1 / (4 scale)), integer grad_x01, grad_cstd = 0, interval
edges multiples of 1/4 (t_mid a multiple of 1/8), origins and directions small dyadic numbers.  One pair then hands its ray
flip_c gx_c / 128 for the origin and that times t_mid for the direction (flip_c = the ray's flip for c = 0, else 1): multiples
of 2^-10 below 2, a ray's sum of up to 190 of them below 2^9.  Pair counts per ray sit at the group's boundaries."""
import functools

import numpy as np

import actor_refs as AR
import packed_restatement as PR

f32, f64 = np.float32, np.float64
LANES = (16, 32, 64, 0)
CUT = (0, 16, 12, 16, 9, 16, 1, 16)  # samples kept per ray of an S = 16 scene, in turn


def chosen_group(n_pairs, n_rays):
    """the group size lanes_per_ray = 0 stands for: the dense rule on the mean pair count (include/neurad_hip.h)"""
    return 64 if n_pairs > 32 * n_rays else (32 if n_pairs > 16 * n_rays else 16)


def log2_group(lanes, n_pairs, n_rays):
    return {16: 4, 32: 5, 64: 6}[lanes or chosen_group(n_pairs, n_rays)]


# ---- GENERIC tier -------------------------------------------------------------------------------------------------------
def production_pairs(sc):
    """the scene's own (sample, actor) pairs in ops.actor_pairs' order, from the float64 containment table"""
    R, S = sc["starts"].shape
    return AR.pairs_of_hits(AR.hits_table(AR.hits64(sc)["inside"].reshape(R * S, -1)))


def random_sorted_pairs(sc, total=1500, seed=77):
    """random distinct (sample, actor) pairs, most of them far outside their box, sorted by (sample, actor)"""
    R, S = sc["starts"].shape
    A = sc["positions"].shape[1]
    key = np.sort(np.random.default_rng(seed).choice(R * S * A, total, replace=False))
    return (key // A).astype(np.int64), (key % A).astype(np.int32)


def cut(sc, si, ai, counts=None):
    """The dense scene as packed rays with the first counts[r] samples of ray r (None: all S, uniform segments).
    -> rays (o, d, area, times, t_starts, t_ends, segments), keep [P] bool: the pairs whose sample survives, and the packed
    sample index of the surviving pairs"""
    R, S = sc["starts"].shape
    counts = np.full(R, S, np.int64) if counts is None else np.asarray(counts, np.int64)
    seg = PR.segments_from_counts(counts)
    kept = np.arange(S)[None, :] < counts[:, None]
    ray, smp = si // S, si % S
    keep = smp < counts[ray]
    rays = (sc["o"], sc["d"], sc["area"], sc["times"], np.ascontiguousarray(sc["starts"][kept]),
            np.ascontiguousarray(sc["ends"][kept]), seg)
    return rays, keep, (seg[ray[keep]] + smp[keep]).astype(np.int64)


def cut_counts(R):
    return np.asarray([CUT[r % len(CUT)] for r in range(R)], np.int64)


def take_rays(rays, pairs, order):
    """The batch with the rays `order` (a permutation, or a subset in any order) and the pairs of those rays, re-indexed and in
    (sample, actor) order again.  rays: (o, d, area, times, ts, te, seg, flip | None); pairs: (si, ai, gx, gs) on packed
    samples -> rays, pairs, `from`: the position each new pair had in the old list"""
    import packed_ray_grad_refs as G

    o, d, area, times, ts, te, seg, flip = rays
    order = np.asarray(order, np.int64)
    (o2, d2, a2, ts2, te2, seg2), take = G.permuted((o, d, area, ts, te, seg), order)
    new_of_old = np.full(len(ts), -1, np.int64)
    new_of_old[take] = np.arange(len(take))
    si, ai, gx, gs = pairs
    nsi = new_of_old[si]
    frm = np.nonzero(nsi >= 0)[0]
    frm = frm[np.argsort(nsi[frm], kind="stable")]  # (pairs of one sample keep their slot order)
    rays2 = (o2, d2, a2, times[order], ts2, te2, seg2, None if flip is None else flip[order])
    return rays2, (nsi[frm], ai[frm], gx[frm], gs[frm]), frm


# ---- EXACT tier ---------------------------------------------------------------------------------------------------------
EXACT_SCALE = 32.0
PER_SAMPLE = 3  # pairs on a sample that has any: three actors share it (the last sample of a ray: what is left)


def exact_counts(G):
    """pairs per ray: the first and the last ray have pairs; -1 marks a ray WITHOUT SAMPLES between two rays with pairs; a
    ray with samples and no pair; the group's boundaries; one long ray; two pairs (one sample, two actors)"""
    return (1, G - 1, -1, G, 0, G + 1, 2 * G + 1, -1, 190, 2)


@functools.lru_cache(maxsize=None)
def exact_case(G):
    """-> dict(actors: timestamps / positions / rotations_6d / present / bounds / scale, rays: (o, d, area, times, ts, te, seg,
    flip), pairs: (si, ai, gx, gs), n_pairs [R], go, gd [R,3] float64: the exact sums)"""
    rng = np.random.default_rng(1000 + G)
    A, Tn = 4, 3
    ts_key = np.array([0.0, 1.0, 2.0], f32)
    pos = np.tile(np.array([[2.0, 0.5, 0.0], [4.0, -0.5, 0.25], [6.0, 0.0, -0.25], [8.0, 1.0, 0.5]], f32)[None], (Tn, 1, 1))
    rot = np.tile(np.asarray(AR.IDENT, f32)[None, None], (Tn, A, 1))
    counts = exact_count_list = exact_counts(G)
    R = len(counts)
    o = np.stack([np.zeros(R), (np.arange(R) % 5 - 2) * 0.5, (np.arange(R) % 3 - 1) * 0.25], -1).astype(f32)
    d = np.tile(np.array([1.0, 0.0, 0.0], f32), (R, 1))
    d[1::2] = (1.0, 0.25, 0.0)  # (not unit length: the pair kernels never normalise a direction)
    times = np.array([-0.5, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 2.5, 0.75, 1.25], f32)[:R]
    flip = np.where(np.arange(R) % 3 == 1, -1.0, 1.0).astype(f32)
    n_samples, si, ai = [], [], []
    first = 0
    for r, n in enumerate(exact_count_list):
        if n < 0:
            n_samples.append(0)
            continue
        with_pairs = -(-n // PER_SAMPLE)
        m = with_pairs + 2  # a leading and a trailing sample no actor claims
        for k in range(n):
            si.append(first + 1 + k // PER_SAMPLE), ai.append(k % PER_SAMPLE + (r % 2))
        n_samples.append(m)
        first += m
    seg = PR.segments_from_counts(n_samples)
    t0 = np.concatenate([0.25 * (1 + np.arange(m)) for m in n_samples]).astype(f32)
    t1 = (t0 + np.concatenate([0.25 * (1 + np.arange(m) % 2) for m in n_samples])).astype(f32)  # widths 1/4 and 1/2
    si, ai = np.asarray(si, np.int64), np.asarray(ai, np.int32)
    P = len(si)
    gx = rng.integers(-8, 9, (P, 3)).astype(f32)
    gs = np.zeros(P, f32)
    ray = PR.ray_indices_from_segments(seg)[si]
    assert si[0] == 1 and ray[0] == 0 and ray[-1] == R - 1 and (np.diff(si) >= 0).all()
    tm = (t0.astype(f64) + (t1.astype(f64) - t0) / 2)[si]
    # the uncontracted branch, everywhere: |box position| < scale in every axis
    mean = o[ray].astype(f64) + d[ray].astype(f64) * tm[:, None]
    assert (np.abs(mean - pos[0, ai].astype(f64)) < EXACT_SCALE).all()
    share = gx.astype(f64) / (4 * EXACT_SCALE)
    share[:, 0] *= flip[ray]
    go, gd = np.zeros((R, 3)), np.zeros((R, 3))
    np.add.at(go, ray, share), np.add.at(gd, ray, share * tm[:, None])
    assert (go == go.astype(f32)).all() and (gd == gd.astype(f32)).all() and np.abs(gd).max() < 2.0 ** 9
    actors = dict(timestamps=ts_key, positions=pos, rotations_6d=rot, present=np.ones((Tn, A), bool),
                  bounds=np.tile(np.array([1.0, 2.0, 2.0], f32), (A, 1)), scale=EXACT_SCALE)
    area = np.full(R, 2.5e-6, f32)
    return dict(actors=actors, rays=(o, d, area, times, t0, t1, seg, flip), pairs=(si, ai, gx, gs),
                n_pairs=np.bincount(ray, minlength=R), go=go, gd=gd)


def exact_as_dense(c):
    """the exact case's pairs as a dense [P,1] scene for grad_edge_refs.actor_pair_grads64: one ray per pair (its own ray's
    constants, its own interval) -> the arguments of that function, and each pair's ray"""
    o, d, area, times, t0, t1, seg, flip = c["rays"]
    si, ai, gx, gs = c["pairs"]
    ray = PR.ray_indices_from_segments(seg)[si]
    a = {k: c["actors"][k] for k in ("positions", "rotations_6d", "timestamps", "scale")}
    P = len(si)
    return (a, o[ray], d[ray], area[ray], t0[si][:, None], t1[si][:, None], times[ray], np.arange(P, dtype=np.int64), ai,
            flip[ray], gx, gs), ray
